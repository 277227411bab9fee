// TEST INFRASTRUCTURE - not part of the product.  The host twin of the `motifs` sweep (deepmod_amd/csrc/motifs.inc: dm_motifs_count_host over
// mok::fate, the routine the kernel of motifs.hip.inc runs per key) under -fsanitize=address,undefined, as a program.  The contig, every table and
// the histogram live in heap blocks of exactly their sizes, so that a read or a write one element outside them is a sanitizer report.  Contigs of
// 0, 1, U + D and U + D + 1 bases at the flanks (8,0), (0,8), (4,4), (0,0) and (3,3); a byte that is none of A, C, G, T at every offset of a
// context; coverage = modified = 2^31 - 1; the refusals.  Every result against a plain restatement of the rules.  tests/test_motifs_host.py builds
// and runs it.
#include "../deepmod_amd/csrc/motifs.inc"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace {

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

int letter_code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

struct Result {
    std::vector<int64_t> hist, counters, off_base;
};

// the rules, restated on std::string and vectors
Result restated(int up, int down, char base, int cov, int t, int u, const std::string& seq, const std::vector<int32_t> tab[4], const std::vector<int32_t>* ctl) {
    Result r{std::vector<int64_t>(size_t(2) << (2 * (up + down)), 0), std::vector<int64_t>(10, 0), std::vector<int64_t>(2, 0)};
    const int n = int(seq.size());
    for (int s = 0; s < 2; ++s)
        for (int p = 0; p < n; ++p) {
            const int own = letter_code(seq[size_t(p)]);
            const int64_t cv = tab[2 * s][size_t(p)], md = tab[2 * s + 1][size_t(p)];
            if (own < 0 || (s ? 3 - own : own) != letter_code(base)) {
                if (cv > 0) ++r.off_base[size_t(s)];
                continue;
            }
            bool edge = false;
            int64_t ctx = 0;
            for (int j = -up; j <= down; ++j) {
                if (j == 0) continue;
                const int q = s ? p - j : p + j;
                const int c = q < 0 || q >= n ? -1 : letter_code(seq[size_t(q)]);
                if (c < 0) edge = true;
                ctx = ctx * 4 + (c < 0 ? 0 : (s ? 3 - c : c));
            }
            int64_t* k = &r.counters[size_t(5 * s)];
            if (edge) {
                ++k[4];
            } else if (cv < cov) {
                ++k[2];
            } else if (ctl && ctl[2 * s][size_t(p)] < cov) {
                ++k[3];
            } else {
                ++k[0];
                ++r.hist[size_t(2 * ctx)];
                const bool quiet = !ctl || 100 * int64_t(ctl[2 * s + 1][size_t(p)]) / int64_t(ctl[2 * s][size_t(p)]) <= u;
                if (100 * md / cv >= t && quiet) {
                    ++k[1];
                    ++r.hist[size_t(2 * ctx + 1)];
                }
            }
        }
    return r;
}

std::unique_ptr<int32_t[]> exact(const std::vector<int32_t>& v) {
    std::unique_ptr<int32_t[]> b(new int32_t[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) b[i] = v[i];
    return b;
}

void one_case(int up, int down, char base, int cov, int t, int u, const std::string& seq, const std::vector<int32_t> tab[4], const std::vector<int32_t>* ctl) {
    const size_t n = seq.size(), bins2 = size_t(2) << (2 * (up + down));
    std::unique_ptr<uint8_t[]> s(new uint8_t[n]);
    for (size_t i = 0; i < n; ++i) s[i] = uint8_t(seq[i]);
    std::unique_ptr<int32_t[]> a[4] = {exact(tab[0]), exact(tab[1]), exact(tab[2]), exact(tab[3])};
    std::unique_ptr<int32_t[]> c[4];
    if (ctl)
        for (int j = 0; j < 4; ++j) c[j] = exact(ctl[j]);
    std::unique_ptr<int64_t[]> hist(new int64_t[bins2]), counters(new int64_t[10]), off(new int64_t[2]);
    for (size_t i = 0; i < bins2; ++i) hist[i] = 0;
    const int rc = dm_motifs_count_host(up, down, base, cov, t, u, s.get(), int64_t(n), a[0].get(), a[1].get(), a[2].get(), a[3].get(), c[0].get(), c[1].get(), c[2].get(),
                                        c[3].get(), hist.get(), counters.get(), off.get());
    CHECK(rc == DM_OK);
    const Result want = restated(up, down, base, cov, t, u, seq, tab, ctl);
    bool same = true;
    for (size_t i = 0; i < bins2; ++i) same = same && hist[i] == want.hist[i];
    for (size_t i = 0; i < 10; ++i) same = same && counters[i] == want.counters[i];
    same = same && off[0] == want.off_base[0] && off[1] == want.off_base[1];
    if (!same) std::printf("differs: flank %d,%d base %c contig %s controls %d\n", up, down, base, seq.c_str(), ctl != nullptr);
    CHECK(same);
}

unsigned g_state = 12345u;
unsigned draw(unsigned n) {
    g_state = g_state * 1664525u + 1013904223u;
    return (g_state >> 8) % n;
}

}  // namespace

int main() {
    const int flanks[][2] = {{8, 0}, {0, 8}, {4, 4}, {0, 0}, {3, 3}, {1, 0}, {0, 1}};
    const int32_t big = 0x7fffffff;
    for (const auto& f : flanks) {
        const int up = f[0], down = f[1], L = up + down;
        for (char base : {'A', 'C', 'G', 'T'})
            for (int n : {0, 1, L, L + 1, 2 * L + 3, 40}) {
                std::string seq(size_t(n), 'A');
                for (auto& ch : seq) ch = "ACGT"[draw(4)];
                std::vector<int32_t> tab[4], ctl[4];
                for (int j = 0; j < 4; ++j) {
                    tab[j].resize(size_t(n));
                    ctl[j].resize(size_t(n));
                }
                for (int s = 0; s < 2; ++s)
                    for (int p = 0; p < n; ++p) {
                        const int32_t covs[] = {0, 4, 5, 6, 100, big};
                        const int32_t cv = covs[draw(6)], ccv = covs[draw(6)];
                        const int32_t mods[] = {0, cv / 2, cv / 2 + 1, cv == 0 ? 0 : cv - 1, cv};
                        const int32_t cmods[] = {0, ccv / 10, ccv / 10 + 1, ccv / 9, ccv};
                        tab[2 * s][size_t(p)] = cv;
                        tab[2 * s + 1][size_t(p)] = mods[draw(5)];
                        ctl[2 * s][size_t(p)] = ccv;
                        ctl[2 * s + 1][size_t(p)] = cmods[draw(5)];
                    }
                one_case(up, down, base, 5, 50, 10, seq, tab, nullptr);
                one_case(up, down, base, 5, 50, 10, seq, tab, ctl);
                one_case(up, down, base, 1, 0, 0, seq, tab, ctl);
                one_case(up, down, base, big, 100, 100, seq, tab, ctl);
                // a byte that is none of A, C, G, T at every offset of the contexts of a base in the middle, on either strand
                if (n == 2 * L + 3) {
                    const int mid = L + 1;
                    for (int j = -L; j <= L; ++j)
                        for (char bad : {'N', 'a', '\0', '\xff'}) {
                            std::string mut = seq;
                            mut[size_t(mid)] = base;
                            if (mid + 1 < n) mut[size_t(mid + 1)] = "TGCA"[letter_code(base)];               // and a base of the '-' strand beside it
                            mut[size_t(mid + j)] = bad;
                            one_case(up, down, base, 5, 50, 10, mut, tab, ctl);
                        }
                }
            }
    }
    // the refusals: nothing is read
    int64_t hist[2] = {0, 0}, counters[10], off[2];
    const uint8_t seq[1] = {'A'};
    const int32_t z[1] = {0};
    CHECK(dm_motifs_count_host(5, 4, 'A', 5, 50, 10, seq, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(-1, 0, 'A', 5, 50, 10, seq, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'N', 5, 50, 10, seq, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'A', 0, 50, 10, seq, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'A', 5, 101, 10, seq, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'A', 5, 50, -1, seq, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'A', 5, 50, 10, seq, 1, z, z, z, z, z, nullptr, z, z, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'A', 5, 50, 10, seq, -1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'A', 5, 50, 10, nullptr, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_EINVAL);
    CHECK(dm_motifs_count_host(0, 0, 'A', 5, 50, 10, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, hist, counters, off) == DM_OK);
    CHECK(hist[0] == 0 && hist[1] == 0);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("MOTIFS-ASAN-OK\n");
    return 0;
}
