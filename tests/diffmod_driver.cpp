// TEST INFRASTRUCTURE - not part of the product.  The host twin of `diffmod` (deepmod_amd/csrc/diffmod.inc: dm_diffmod_test_host over dfk::fate and
// dfk::fisher_p, the routines the kernels of diffmod.hip.inc run per key) under -fsanitize=address,undefined, as a program.  Every table, the
// histogram and every record array live in heap blocks of exactly their sizes, so that a read or a write one element outside them is a sanitizer
// report; so does the table of lgamma inside the twin (a std::vector of MAX_TOTAL + 1 doubles), which a key at MAX_TOTAL reads to its last entry.
// Contigs of 0, 1, TILE - 1, TILE, TILE + 1 and 3 TILE + 5 positions (TILE = 1024, the tile of the select kernel) carrying the supports 1, 2, 16,
// 17, 64, 65, 256, 257 and 5001, a key at MAX_TOTAL and one above it, every fate on both strands, and modified counts outside 0..coverage, which the
// routines hold to that range.  Fates and record order against a plain restatement; p against closed forms and the symmetries.
// tests/test_diffmod_host.py builds and runs it.
#include "../deepmod_amd/csrc/diffmod.inc"

#include <cstdio>
#include <cstdlib>
#include <memory>
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

constexpr int TILE = 1024, COV = 5, MAXT = 1 << 20;

struct Key {
    int32_t cA, mA, cB, mB;
};

Key with_support(int S, double share) {
    const int M = S - 1, mA = int(share * M + 0.5);
    return {M + 5, mA, M + 5, M - mA};
}

std::vector<Key> keys() {
    std::vector<Key> k;
    for (int S : {1, 2, 16, 17, 64, 65, 256, 257}) k.push_back(with_support(S, 0.6));
    k.push_back({5000, 2600, 5000, 2400});
    k.push_back({5000, 5000, 5000, 0});
    k.push_back({MAXT / 2, 30, MAXT / 2, 10});
    k.push_back({MAXT - 6, 3, 6, 2});
    k.push_back({MAXT / 2 + 1, 30, MAXT / 2, 10});                     // too_deep
    k.push_back({0x7fffffff, 0, 0x7fffffff, 0});                       // too_deep: the sum is formed in 64 bits
    k.push_back({COV - 1, 1, 30, 3});
    k.push_back({0, 0, 30, 3});
    k.push_back({30, 3, COV - 1, 0});
    k.push_back({30, 3, 0, 0});
    k.push_back({0, 0, 0, 0});
    k.push_back({9, 9, 9, 9});
    k.push_back({9, 12, 9, -4});                                       // held to 9, 9, 9, 0
    return k;
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> b(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) b[i] = v[i];
    return b;
}

int restated_fate(const Key& k) {
    if (k.cA == 0 && k.cB == 0) return -1;
    if (k.cA < COV) return 1;
    if (k.cB < COV) return 2;
    if (int64_t(k.cA) + int64_t(k.cB) > MAXT) return 3;
    return 0;
}

void one_contig(int64_t n, int phase, double alpha) {
    const std::vector<Key> ks = keys();
    std::vector<int32_t> tab[8];                                       // cov+, mod+, cov-, mod-, and the controls' four
    for (auto& t : tab) t.assign(size_t(n), 0);
    int64_t want[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tested = 0;
    for (int64_t q = 0; q < n; ++q)
        for (int s = 0; s < 2; ++s) {
            const bool spot = q == 0 || q == n - 1 || q % TILE == 0 || q % TILE == TILE - 1 || q % 37 == phase;
            if (!spot) continue;
            const Key& k = ks[size_t((2 * q + s + phase) % int64_t(ks.size()))];
            tab[2 * s][size_t(q)] = k.cA;
            tab[2 * s + 1][size_t(q)] = k.mA;
            tab[4 + 2 * s][size_t(q)] = k.cB;
            tab[4 + 2 * s + 1][size_t(q)] = k.mB;
            const int f = restated_fate(k);
            if (f >= 0) ++want[4 * s + f];
            tested += f == 0;
        }
    std::unique_ptr<int32_t[]> a[8];
    for (int j = 0; j < 8; ++j) a[j] = exact(tab[j]);
    std::unique_ptr<int64_t[]> counters(new int64_t[8]), hist(new int64_t[20]), n_rec(new int64_t[1]);
    for (int j = 0; j < 20; ++j) hist[j] = 0;
    const int64_t cap = tested;                                        // alpha 1: exactly every tested key
    std::unique_ptr<int32_t[]> pos(new int32_t[size_t(cap)]), cA(new int32_t[size_t(cap)]), mA(new int32_t[size_t(cap)]), cB(new int32_t[size_t(cap)]), mB(new int32_t[size_t(cap)]);
    std::unique_ptr<uint8_t[]> strand(new uint8_t[size_t(cap)]);
    std::unique_ptr<double[]> p(new double[size_t(cap)]);
    const int rc = dm_diffmod_test_host(COV, alpha, n, a[0].get(), a[1].get(), a[2].get(), a[3].get(), a[4].get(), a[5].get(), a[6].get(), a[7].get(), counters.get(),
                                        hist.get(), cap, pos.get(), strand.get(), cA.get(), mA.get(), cB.get(), mB.get(), p.get(), n_rec.get());
    CHECK(rc == DM_OK);
    for (int j = 0; j < 8; ++j) CHECK(counters[j] == want[j]);
    int64_t in_hist = 0;
    for (int j = 0; j < 20; ++j) in_hist += hist[j];
    CHECK(in_hist == tested);
    CHECK(n_rec[0] <= tested && (alpha < 1.0 || n_rec[0] == tested));
    for (int64_t i = 0; i < n_rec[0] && i < cap; ++i) {
        CHECK(p[i] >= 0.0 && p[i] <= alpha);
        CHECK(i == 0 || 2 * int64_t(pos[i - 1]) + strand[i - 1] < 2 * int64_t(pos[i]) + strand[i]);          // key order
        CHECK(mA[i] >= 0 && mA[i] <= cA[i] && mB[i] >= 0 && mB[i] <= cB[i]);
        CHECK(cA[i] == tab[2 * strand[i]][size_t(pos[i])] && cB[i] == tab[4 + 2 * strand[i]][size_t(pos[i])]);
    }
}

bool close(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fabs(b); }

}  // namespace

int main() {
    for (int64_t n : {int64_t(0), int64_t(1), int64_t(TILE - 1), int64_t(TILE), int64_t(TILE + 1), int64_t(3 * TILE + 5)})
        for (int phase : {0, 1, 5}) {
            one_contig(n, phase, 1.0);
            one_contig(n, phase, 0.05);
        }
    // p: closed forms and the symmetries
    const double* lf = dfk::lf_table();
    CHECK(lf[0] == 0.0 && lf[1] == 0.0 && close(lf[dfk::MAX_TOTAL], 13487781.810466923, 1e-15));
    CHECK(close(dfk::fisher_p(lf, 5, 5, 5, 0), 2.0 / 252.0, 1e-12));
    CHECK(close(dfk::fisher_p(lf, 3, 1, 3, 2), 1.0, 1e-12));
    CHECK(dfk::fisher_p(lf, 9, 9, 9, 9) == 1.0 && dfk::fisher_p(lf, 9, 0, 7, 0) == 1.0 && dfk::fisher_p(lf, 9, 12, 9, 40) == 1.0);
    CHECK(dfk::fisher_p(lf, 5000, 5000, 5000, 0) == 0.0);
    for (const Key& k : keys()) {
        if (restated_fate(k) != 0) continue;
        const int mA = dfk::held(k.mA, k.cA), mB = dfk::held(k.mB, k.cB);
        const double p = dfk::fisher_p(lf, k.cA, mA, k.cB, mB);
        const double rel = int64_t(k.cA) + k.cB <= 4096 ? 2e-9 : 2e-6;                                     // twice the bound: both sides carry it
        CHECK(p >= 0.0 && p <= 1.0);
        CHECK(close(dfk::fisher_p(lf, k.cB, mB, k.cA, mA), p, rel) || p == 0.0);                           // sample and control swapped
        CHECK(close(dfk::fisher_p(lf, k.cA, k.cA - mA, k.cB, k.cB - mB), p, rel) || p == 0.0);             // modified and unmodified swapped
    }
    // the refusals: nothing is read
    int64_t counters[8], hist[20] = {}, n_rec = -1;
    const int32_t z[1] = {0};
    CHECK(dm_diffmod_test_host(0, 0.05, 1, z, z, z, z, z, z, z, z, counters, hist, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_rec) == DM_EINVAL);
    CHECK(dm_diffmod_test_host(5, 0.0, 1, z, z, z, z, z, z, z, z, counters, hist, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_rec) == DM_EINVAL);
    CHECK(dm_diffmod_test_host(5, 1.5, 1, z, z, z, z, z, z, z, z, counters, hist, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_rec) == DM_EINVAL);
    CHECK(dm_diffmod_test_host(5, 0.05, 1, z, z, z, z, nullptr, nullptr, nullptr, nullptr, counters, hist, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               &n_rec) == DM_EINVAL);
    CHECK(dm_diffmod_test_host(5, 0.05, 1, z, z, z, z, z, z, nullptr, z, counters, hist, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_rec) == DM_EINVAL);
    CHECK(dm_diffmod_test_host(5, 0.05, -1, z, z, z, z, z, z, z, z, counters, hist, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_rec) == DM_EINVAL);
    CHECK(dm_diffmod_test_host(5, 0.05, 1, z, z, z, z, z, z, z, z, counters, hist, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_rec) == DM_EINVAL);
    CHECK(n_rec == -1);
    CHECK(dm_diffmod_test_host(5, 0.05, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, counters, hist, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, &n_rec) == DM_OK);
    CHECK(n_rec == 0 && counters[0] == 0 && hist[19] == 0);
    CHECK(dm_diffmod_max_total() == MAXT);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("DIFFMOD-DRIVER-OK\n");
    return 0;
}
