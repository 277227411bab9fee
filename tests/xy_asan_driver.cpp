// TEST INFRASTRUCTURE - not part of the product.  The host part of getfeatures (deepmod_amd/csrc/xyrows.inc: dm_xy_read, dm_xy_labels, dm_xy_rows_host,
// dm_xy_format_host) under -fsanitize=address,undefined, as a program: tests/asan/host_shim.cpp (the host part of the C ABI, compiled by g++) is included as
// it is, xyrows.inc behind it, and every array of every call lives in a heap block of exactly its size, so that a read or a write one element outside
// it is a sanitizer report.  Valid batches against a plain restatement of the selection, damaged descriptor tables, CIGARs that run past their
// sequences, output arrays that are too small.  tests/test_getfeatures_host.py builds and runs it.
#include "asan/host_shim.cpp"

#include "../deepmod_amd/csrc/xyrows.inc"

#include <cstdlib>
#include <memory>
#include <random>

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

struct Batch {
    std::vector<int64_t> pos, rdesc;
    std::vector<uint8_t> lab, code;
    std::vector<float> ev3;
    int64_t n_reads = 0, n_rows = 0, n_events = 0;
};

Batch make_batch(std::mt19937_64& rng, int n_reads) {
    Batch b;
    for (int r = 0; r < n_reads; ++r) {
        const int64_t rows = 1 + int64_t(rng() % 300), ev = int64_t(rng() % 260), shift = int64_t(rng() % 120) - 60;
        b.rdesc.insert(b.rdesc.end(), {b.n_rows, b.n_events + shift - b.n_rows, b.n_events, b.n_events + ev});
        for (int64_t q = 0; q < rows; ++q) {
            b.pos.push_back(int64_t(rng() % 1000000));
            b.lab.push_back(rng() % 40 == 0 ? uint8_t(1 + rng() % 2) : 0);
            b.code.push_back(uint8_t(rng() % 5 == 4 ? 255 : rng() % 4));
        }
        for (int64_t e = 0; e < ev; ++e) b.ev3.insert(b.ev3.end(), {float(int(rng() % 9000) - 4500) / 1000.0f, float(rng() % 900) / 1000.0f, float(1 + rng() % 60)});
        b.n_rows += rows;
        b.n_events += ev;
    }
    b.n_reads = n_reads;
    return b;
}

// dm_xy_rows_host with every array in a block of its own size -> (bytes or error, keep, row_off, text)
struct Out {
    int64_t rc;
    std::vector<uint8_t> keep;
    std::vector<int64_t> row_off, byte_off;
    std::string text;
};

Out run(const Batch& b, const std::vector<int64_t>& rdesc) {
    auto pos = exact(b.pos);
    auto lab = exact(b.lab);
    auto code = exact(b.code);
    auto rd = exact(rdesc);
    auto ev3 = exact(b.ev3);
    std::unique_ptr<uint8_t[]> keep(new uint8_t[b.n_rows]);
    std::unique_ptr<int64_t[]> ro(new int64_t[b.n_reads + 1]), bo(new int64_t[b.n_reads + 1]);
    Out o;
    o.rc = dm_xy_rows_host(pos.get(), lab.get(), code.get(), rd.get(), b.n_reads, b.n_rows, ev3.get(), b.n_events, keep.get(), ro.get(), bo.get(), nullptr, 0);
    if (o.rc < 0) return o;
    std::unique_ptr<char[]> text(new char[o.rc]);
    CHECK(dm_xy_rows_host(pos.get(), lab.get(), code.get(), rd.get(), b.n_reads, b.n_rows, ev3.get(), b.n_events, nullptr, nullptr, nullptr, text.get(), o.rc) == o.rc);
    if (o.rc > 1) {                                                  // a buffer one byte short is filled as far as it reaches, never beyond
        std::unique_ptr<char[]> shorter(new char[o.rc - 1]);
        CHECK(dm_xy_rows_host(pos.get(), lab.get(), code.get(), rd.get(), b.n_reads, b.n_rows, ev3.get(), b.n_events, nullptr, nullptr, nullptr, shorter.get(), o.rc - 1) == o.rc);
    }
    o.keep.assign(keep.get(), keep.get() + b.n_rows);
    o.row_off.assign(ro.get(), ro.get() + b.n_reads + 1);
    o.byte_off.assign(bo.get(), bo.get() + b.n_reads + 1);
    o.text.assign(text.get(), text.get() + o.rc);
    return o;
}

}  // namespace

int main() {
    std::mt19937_64 rng(11);
    int n_valid = 0, n_refused = 0;
    for (int it = 0; it < 300; ++it) {
        const Batch b = make_batch(rng, 1 + int(rng() % 5));
        const Out o = run(b, b.rdesc);
        CHECK(o.rc >= 0);
        if (o.rc < 0) continue;
        ++n_valid;
        // the selection, restated: quadratic and plain
        int64_t out_rows = 0, lines = 0;
        for (int64_t r = 0; r < b.n_reads; ++r) {
            const int64_t r0 = b.rdesc[4 * r], r1 = r + 1 < b.n_reads ? b.rdesc[4 * (r + 1)] : b.n_rows;
            std::vector<uint8_t> k(size_t(r1 - r0), 0);
            int64_t kept = 0;
            for (int64_t q = r0; q < r1; ++q) {
                for (int64_t j = std::max(r0, q - 25); j <= std::min(r1 - 1, q + 25); ++j)
                    if (b.lab[size_t(j)]) k[size_t(q - r0)] = 1;
                kept += k[size_t(q - r0)];
            }
            if (kept > 0 && double(kept) > double(r1 - r0) * 0.9) {
                std::fill(k.begin(), k.end(), 1);
                kept = r1 - r0;
            }
            CHECK(o.row_off[size_t(r)] == out_rows);
            for (int64_t q = r0; q < r1; ++q) CHECK(o.keep[size_t(q)] == k[size_t(q - r0)]);
            out_rows += kept;
        }
        CHECK(o.row_off[size_t(b.n_reads)] == out_rows);
        for (char c : o.text) lines += c == '\n';
        CHECK(lines == out_rows && o.byte_off[size_t(b.n_reads)] == o.rc);
        // one damaged entry of the descriptor table: refused, or still inside every array (the sanitizer watches)
        for (int k = 0; k < 12; ++k) {
            std::vector<int64_t> bad = b.rdesc;
            const size_t at = size_t(rng() % bad.size());
            const int64_t vals[] = {-1, INT64_MIN, INT64_MAX, b.n_rows, b.n_rows + 1, b.n_events + 1, int64_t(1) << 45, -(int64_t(1) << 45), bad[at] + 1, bad[at] - 1};
            bad[at] = vals[rng() % 10];
            const Out d = run(b, bad);
            if (d.rc < 0) {
                CHECK(d.rc == DM_EINVAL);
                ++n_refused;
            }
        }
    }
    // the text definition: sized first, nothing written into a buffer that is too small
    {
        const std::vector<double> rows = {0, 1, 0, 0, 1, 0, 0, -0.0004, 9.9996, 16777216.0, 1e300, NAN, -INFINITY, 0.0625, 2.6875, -2.6875, 0, 0, 0, 0.0005};
        auto r = exact(rows);
        const int64_t need = dm_xy_format_host(r.get(), 2, nullptr, 0);
        CHECK(need > 300);
        std::unique_ptr<char[]> out(new char[need]), shorter(new char[need - 1]);
        CHECK(dm_xy_format_host(r.get(), 2, out.get(), need) == need && out[need - 1] == '\n');
        CHECK(dm_xy_format_host(r.get(), 2, shorter.get(), need - 1) == need);
        CHECK(std::string(out.get(), size_t(need)).find(" nan -inf 0.062 2.688 -2.688 0.000 0.000 0.000 0.001\n") != std::string::npos);
    }
    // the walk: reference, read and outputs in blocks of their own size
    {
        std::string ref;
        for (int i = 0; i < 900; ++i) ref.push_back("ACGT"[rng() % 4]);
        const std::string read = ref.substr(100, 620);
        dm_xysites* s = dm_xy_sites_create(1, 0, 0);
        std::vector<int64_t> sites;
        for (int64_t i = 0; i + 1 < int64_t(ref.size()); ++i)
            if (ref[size_t(i)] == 'C' && ref[size_t(i) + 1] == 'G') sites.push_back(i);
        CHECK(dm_xy_sites_set(s, 0, 0, 0, sites.data(), int64_t(sites.size())) == DM_OK);
        CHECK(dm_xy_sites_set(s, 1, 0, 0, sites.data(), 1) == DM_EINVAL && dm_xy_sites_set(s, 0, 2, 0, sites.data(), 1) == DM_EINVAL);
        auto rf = exact(std::vector<char>(ref.begin(), ref.end()));
        auto rd = exact(std::vector<char>(read.begin(), read.end()));
        const int64_t rows = 620 + 200;
        std::unique_ptr<int64_t[]> pos(new int64_t[rows]);
        std::unique_ptr<uint8_t[]> lab(new uint8_t[rows]), code(new uint8_t[rows]);
        int64_t rdesc[4], info[DM_XY_INFO_LEN];
        for (int posneg = 0; posneg < 2; ++posneg) {
            CHECK(dm_xy_read(s, 0, 0, 101, "620M", rd.get(), 620, rf.get(), 900, 620, "CG", 0, posneg, pos.get(), lab.get(), code.get(), rows, 0, 0, rdesc, info) == DM_OK);
            CHECK(info[DM_XY_STATUS] == DM_XY_OK && info[DM_XY_N_ROWS] == rows && pos[100] == 100 && pos[719] == 719 && pos[720] == 0);
        }
        // one row too few: nothing is written
        CHECK(dm_xy_read(s, 0, 0, 101, "620M", rd.get(), 620, rf.get(), 900, 620, "CG", 0, 1, pos.get(), lab.get(), code.get(), rows - 1, 0, 0, rdesc, info) == DM_OK);
        CHECK(info[DM_XY_STATUS] == DM_XY_NEED_ROWS && info[DM_XY_N_ROWS] == rows);
        // CIGARs that run past the read / the reference, more events than bases, a motif position outside the motif
        CHECK(dm_xy_read(s, 0, 0, 101, "621M", rd.get(), 620, rf.get(), 900, 620, "CG", 0, 1, pos.get(), lab.get(), code.get(), rows, 0, 0, rdesc, info) == DM_EINVAL);
        CHECK(dm_xy_read(s, 0, 0, 301, "620M", rd.get(), 620, rf.get(), 900, 620, "CG", 0, 1, pos.get(), lab.get(), code.get(), rows, 0, 0, rdesc, info) == DM_EINVAL);
        CHECK(dm_xy_read(s, 0, 0, 101, "620M", rd.get(), 620, rf.get(), 900, 620, "CG", 2, 1, pos.get(), lab.get(), code.get(), rows, 0, 0, rdesc, info) == DM_EINVAL);
        CHECK(dm_xy_read(s, 0, 16, 101, "10S600M10S", rd.get(), 620, rf.get(), 900, 620, "CG", 0, 1, pos.get(), lab.get(), code.get(), rows, 0, 0, rdesc, info) == DM_OK);
        CHECK(info[DM_XY_STATUS] == DM_XY_NO_MATCH || info[DM_XY_STATUS] == DM_XY_LESS_EVENT || info[DM_XY_STATUS] == DM_XY_OK);
        CHECK(dm_xy_read(s, 0, 0, 101, "499M121S", rd.get(), 620, rf.get(), 900, 620, "CG", 0, 1, pos.get(), lab.get(), code.get(), rows, 0, 0, rdesc, info) == DM_OK);
        CHECK(info[DM_XY_STATUS] == DM_XY_LESS_EVENT);
        // a table with fewer read bases than aligned events
        {
            const std::vector<char> tb = {'A', 'C', 'G', 'T'}, qb = {'A', '-', 'G', 'T'};
            const std::vector<uint64_t> ti = {5, 6, 7, 8};
            auto a = exact(tb);
            auto q = exact(qb);
            auto i = exact(ti);
            std::unique_ptr<int64_t[]> p2(new int64_t[204]);
            std::unique_ptr<uint8_t[]> l2(new uint8_t[204]), c2(new uint8_t[204]);
            CHECK(dm_xy_labels(s, 0, 0, "CG", 0, 1, a.get(), q.get(), i.get(), 4, 4, 0, 0, 5, 0, p2.get(), l2.get(), c2.get(), 204, 0, 0, rdesc, info) == DM_OK);
            CHECK(info[DM_XY_STATUS] == DM_XY_INDEX_ERROR);
            CHECK(dm_xy_labels(s, 0, 0, "CG", 0, 1, a.get(), q.get(), i.get(), 4, 3, 0, 0, 5, 0, p2.get(), l2.get(), c2.get(), 203, 0, 0, rdesc, info) == DM_OK);
            CHECK(info[DM_XY_STATUS] == DM_XY_OK && info[DM_XY_N_ROWS] == 203 && p2[100] == 5 && p2[101] == 7 && p2[102] == 8);
            CHECK(dm_xy_labels(s, 0, 0, "CG", 0, 1, a.get(), q.get(), i.get(), 4, 3, 5, 0, 5, 0, p2.get(), l2.get(), c2.get(), 203, 0, 0, rdesc, info) == DM_OK);
            CHECK(info[DM_XY_STATUS] == DM_XY_INDEX_ERROR);
        }
        dm_xy_sites_destroy(s);
    }
    CHECK(n_valid == 300 && n_refused > 500);
    if (g_failed) return 1;
    std::printf("XY-ASAN-OK valid %d refused %d\n", n_valid, n_refused);
    return 0;
}
