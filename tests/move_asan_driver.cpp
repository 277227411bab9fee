// TEST INFRASTRUCTURE - not part of the product.  dm_move_events (deepmod_amd/csrc/rowsbatch.inc) under -fsanitize=address,undefined, as a program:
// tests/asan/host_shim.cpp (the host part of the C ABI, compiled by g++) is included as it is, and every table of every call lives in a heap block of
// exactly its size, so that a read or a write one element outside it is a sanitizer report.  Valid reads, the cases where the reference is undefined,
// damaged offset tables and random tables against a plain restatement.  tests/test_move.py builds and runs it.
#include "asan/host_shim.cpp"

#include <cstdlib>
#include <memory>
#include <random>

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a block of exactly v.size() elements (new T[0] is a valid, unreadable block)
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

struct Result {
    int64_t rc;
    std::vector<int64_t> mev_off;
    std::vector<int32_t> status;
    std::vector<uint64_t> start, length;
    std::string bases;
};

Result run(const std::vector<uint8_t>& move, const std::vector<int64_t>& mv_off, const std::vector<int64_t>& first, const std::vector<int64_t>& raw_off,
           const std::string& fq, const std::vector<int64_t>& fq_off, int64_t n_move = -1, int64_t n_fq = -1) {
    const int64_t n = int64_t(first.size());
    auto mv = exact(move);
    auto mo = exact(mv_off);
    auto fs = exact(first);
    auto ro = exact(raw_off);
    auto sq = exact(std::vector<char>(fq.begin(), fq.end()));
    auto fo = exact(fq_off);
    std::unique_ptr<int64_t[]> mev(new int64_t[n + 1]);
    std::unique_ptr<int32_t[]> st(new int32_t[n]);
    std::unique_ptr<uint64_t[]> s(new uint64_t[fq.size()]), l(new uint64_t[fq.size()]);
    std::unique_ptr<char[]> b(new char[fq.size()]);
    Result r;
    r.rc = dm_move_events(n, n_move < 0 ? int64_t(move.size()) : n_move, mv.get(), mo.get(), fs.get(), ro.get(), n_fq < 0 ? int64_t(fq.size()) : n_fq, sq.get(),
                          fo.get(), mev.get(), st.get(), s.get(), l.get(), b.get());
    if (r.rc >= 0) {
        r.mev_off.assign(mev.get(), mev.get() + n + 1);
        r.status.assign(st.get(), st.get() + n);
        r.start.assign(s.get(), s.get() + r.rc);
        r.length.assign(l.get(), l.get() + r.rc);
        r.bases.assign(b.get(), b.get() + r.rc);
    }
    return r;
}

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

}  // namespace

int main() {
    using V8 = std::vector<uint8_t>;
    using V64 = std::vector<int64_t>;
    // one valid read
    {
        Result r = run(V8{1, 0, 1, 0, 0, 1, 2, 1}, V64{0, 8}, V64{3}, V64{0, 40}, "ACGT", V64{0, 4});
        CHECK(r.rc == 4 && r.status[0] == DM_MOVE_OK);
        CHECK((r.start == std::vector<uint64_t>{3, 7, 13, 17}) && (r.length == std::vector<uint64_t>{4, 6, 4, 23}) && r.bases == "ACGT");
    }
    // the undefined cases: a status, no events, nothing written
    CHECK(run(V8{1, 1, 0, 1, 1, 0}, V64{0, 6}, V64{4}, V64{0, 40}, "ACG", V64{0, 3}).status[0] == DM_MOVE_COUNT);
    CHECK(run(V8{1, 0, 0, 1, 0, 0}, V64{0, 6}, V64{4}, V64{0, 40}, "ACG", V64{0, 3}).status[0] == DM_MOVE_COUNT);
    CHECK(run(V8{}, V64{0, 0}, V64{4}, V64{0, 40}, "ACG", V64{0, 3}).status[0] == DM_MOVE_COUNT);
    CHECK(run(V8{1, 0, 0}, V64{0, 3}, V64{4}, V64{0, 40}, "", V64{0, 0}).status[0] == DM_MOVE_COUNT);
    CHECK(run(V8{1, 0, 1, 0, 0, 1}, V64{0, 6}, V64{4}, V64{0, 14}, "ACG", V64{0, 3}).status[0] == DM_MOVE_OUTSIDE);
    CHECK(run(V8{1, 0, 1, 0, 0, 1}, V64{0, 6}, V64{4}, V64{0, 15}, "ACG", V64{0, 3}).status[0] == DM_MOVE_OK);
    CHECK(run(V8{1, 0, 1, 0, 0, 1}, V64{0, 6}, V64{40}, V64{0, 40}, "ACG", V64{0, 3}).status[0] == DM_MOVE_OUTSIDE);
    CHECK(run(V8{1, 0, 1, 0, 0, 1}, V64{0, 6}, V64{-1}, V64{0, 40}, "ACG", V64{0, 3}).status[0] == DM_MOVE_OUTSIDE);
    CHECK(run(V8{1, 0, 1, 0, 0, 1}, V64{0, 6}, V64{INT64_MIN}, V64{0, 40}, "ACG", V64{0, 3}).status[0] == DM_MOVE_OUTSIDE);
    CHECK(run(V8{1, 0, 1, 0, 0, 1}, V64{0, 6}, V64{INT64_MAX}, V64{0, 40}, "ACG", V64{0, 3}).status[0] == DM_MOVE_OUTSIDE);
    CHECK(run(V8{1}, V64{0, 1}, V64{0}, V64{0, 0}, "A", V64{0, 1}).status[0] == DM_MOVE_OUTSIDE);
    // damaged offset tables: an error code before a byte is read
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, 7}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 4}).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 4, 3}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 4}).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{-2, 3, 6}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 4}).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, INT64_MAX}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 4}).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, 6}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 5}).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, 6}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 3, 2}).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, 6}, V64{2, 3}, V64{0, 20, 10}, "ACGT", V64{0, 2, 4}).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, 6}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 4}, 5).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, 6}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 4}, -1, 3).rc == DM_EINVAL);
    CHECK(run(V8{1, 0, 1, 0, 1, 0}, V64{0, 3, 6}, V64{2, 3}, V64{0, 20, 40}, "ACGT", V64{0, 2, 4}).rc == 4);
    // random containers: valid and invalid reads mixed, against a plain restatement
    std::mt19937_64 rng(7);
    int n_ok = 0, n_bad = 0;
    for (int it = 0; it < 400; ++it) {
        const int n = int(rng() % 6);
        V8 move;
        V64 mv_off{0}, first, raw_off{0}, fq_off{0};
        std::string fq;
        std::vector<uint64_t> want_start, want_len;
        std::vector<int32_t> want_status;
        for (int r = 0; r < n; ++r) {
            const int len = int(rng() % 40);
            V8 t(len);
            int nb = 0, last = 0;
            for (int i = 0; i < len; ++i) {
                t[i] = uint8_t(rng() % 7 < 2 ? 1 : rng() % 5 == 0 ? 2 : 0);
                if (i >= 1 && t[i] == 1) {
                    ++nb;
                    last = i;
                }
            }
            const int kind = int(rng() % 8);
            const int nrow = kind == 0 ? nb + 2 : kind == 1 ? nb : nb + 1;      // too few / too many boundaries for the bases / as many as needed
            const int64_t f = kind == 2 ? -int64_t(rng() % 3) - 1 : int64_t(rng() % 9);
            int64_t nsig = f + 2 * last + 1 + int64_t(rng() % 5);
            if (kind == 3) nsig = f + 2 * last - int64_t(rng() % 3);              // the last event would be empty or start outside
            if (nsig < 0) nsig = 0;
            move.insert(move.end(), t.begin(), t.end());
            mv_off.push_back(int64_t(move.size()));
            first.push_back(f);
            raw_off.push_back(raw_off.back() + nsig);
            for (int k = 0; k < nrow; ++k) fq.push_back("ACGT"[rng() % 4]);
            fq_off.push_back(int64_t(fq.size()));
            int32_t st = DM_MOVE_OK;
            if (nb != nrow - 1) st = DM_MOVE_COUNT;
            else if (f < 0 || f >= nsig || (nb > 0 && f + 2 * last >= nsig)) st = DM_MOVE_OUTSIDE;
            want_status.push_back(st);
            if (st == DM_MOVE_OK) {
                uint64_t pivot = uint64_t(f);
                for (int i = 1; i < len; ++i)
                    if (t[i] == 1) {
                        want_start.push_back(pivot);
                        want_len.push_back(uint64_t(f + 2 * i) - pivot);
                        pivot = uint64_t(f + 2 * i);
                    }
                want_start.push_back(pivot);
                want_len.push_back(uint64_t(nsig) - pivot);
                ++n_ok;
            } else {
                ++n_bad;
            }
        }
        Result r = run(move, mv_off, first, raw_off, fq, fq_off);
        CHECK(r.rc == int64_t(want_start.size()));
        CHECK(r.status == want_status && r.start == want_start && r.length == want_len);
        for (uint64_t v : r.length) CHECK(v > 0);
    }
    CHECK(n_ok > 100 && n_bad > 100);
    if (g_failed) return 1;
    std::printf("MOVE-ASAN-OK valid %d invalid %d\n", n_ok, n_bad);
    return 0;
}
