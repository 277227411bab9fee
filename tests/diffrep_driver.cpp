// TEST INFRASTRUCTURE - not part of the product.  The host twin of `diffmod --replicates 1` (deepmod_amd/csrc/diffrep.inc: dm_diffrep_test_host over
// dfr::test_key, the routine the kernel of diffrep.hip.inc runs per key) under -fsanitize=address,undefined, as a program.  Every table, the pointer
// lists, the histogram and every record array live in heap blocks of exactly their sizes, so that a read or a write one element outside them is a
// sanitizer report.  Contigs of 0, 1, TILE - 1, TILE, TILE + 1 and 3 TILE + 5 positions (TILE = 1024, the tile of the sweep) at (1, 2), (2, 1),
// (3, 5) and (8, 8) replicates: every fate on both strands, a replicate below cov and one absent, a key at MAX_TOTAL and one above it, coverages whose
// sum needs 64 bits, and modified counts outside 0..coverage, which the routine holds to that range.  Fates and record order against a plain
// restatement; the F tail against its closed forms for nu = 1, 2 and 4.  tests/test_diffrep_host.py builds and runs it.
#include "../deepmod_amd/csrc/diffrep.inc"

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
    std::vector<int32_t> c, m;
};

// the keys of a shape: replicate j of n gets c[j], m[j]
std::vector<Key> keys(int n_a, int n_b) {
    const int K = n_a + n_b;
    std::vector<Key> k;
    auto both = [&](int ca, int ma, int cb, int mb) {
        Key x;
        for (int j = 0; j < K; ++j) x.c.push_back(j < n_a ? ca : cb), x.m.push_back(j < n_a ? ma : mb);
        return x;
    };
    k.push_back(both(10, 3, 20, 6));                                   // equal by the integer rule
    k.push_back(both(30, 0, 25, 25));
    k.push_back(both(40, 10, 40, 25));
    Key odd = both(100, 5, 100, 95);
    for (int j = 0; j < K; j += 2) odd.m[size_t(j)] = 60;              // far overdispersed
    k.push_back(odd);
    Key low = both(40, 10, 40, 25);
    low.c[0] = COV - 1, low.m[0] = 1;                                  // a replicate below cov
    k.push_back(low);
    Key gone = both(40, 10, 40, 25);
    gone.c[size_t(K - 1)] = 0, gone.m[size_t(K - 1)] = 0;              // a replicate absent
    k.push_back(gone);
    Key at = both(MAXT / 2 / n_a, 1000, (MAXT - (MAXT / 2 / n_a) * n_a) / n_b, 2000);
    at.c[size_t(K - 1)] += MAXT - ((MAXT / 2 / n_a) * n_a + ((MAXT - (MAXT / 2 / n_a) * n_a) / n_b) * n_b);          // exactly MAX_TOTAL
    k.push_back(at);
    Key above = at;
    above.c[0] += 1;                                                   // too_deep
    k.push_back(above);
    k.push_back(both(0x7fffffff, 7, 0x7fffffff, 9));                   // too_deep: the sum is formed in 64 bits
    k.push_back(both(20, 35, 20, -4));                                 // held to 20 and 0
    k.push_back(both(0, 0, 0, 0));
    k.push_back(both(0, 0, 30, 3));                                    // no sample replicate
    k.push_back(both(30, 3, 0, 0));
    k.push_back(both(30, 3, COV - 1, 2));
    return k;
}

int restated_fate(const Key& k, int n_a, int min_a, int min_b, int64_t* sums /* cA mA cB mB nA nB */) {
    bool any = false;
    for (int j = 0; j < 6; ++j) sums[j] = 0;
    for (size_t j = 0; j < k.c.size(); ++j) {
        const int64_t c = k.c[j] > 0 ? k.c[j] : 0;
        any = any || c > 0;
        if (c < COV) continue;
        const int64_t m = k.m[j] < 0 ? 0 : (k.m[j] > c ? c : k.m[j]);
        const int g = int(j) < n_a ? 0 : 1;
        sums[2 * g] += c, sums[2 * g + 1] += m, sums[4 + g] += 1;
    }
    if (!any) return -1;
    if (sums[4] < min_a) return 1;
    if (sums[5] < min_b) return 2;
    if (sums[0] + sums[2] > MAXT) return 3;
    return 0;
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> b(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) b[i] = v[i];
    return b;
}

void one_contig(int n_a, int n_b, int min_a, int min_b, int64_t n, int phase, double alpha) {
    const std::vector<Key> ks = keys(n_a, n_b);
    const int K = n_a + n_b;
    std::vector<std::vector<int32_t>> tab(size_t(4 * K));              // replicate j: cov+, mod+, cov-, mod- at 4 j ..
    for (auto& t : tab) t.assign(size_t(n), 0);
    int64_t want[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tested = 0, sums[6];
    std::vector<int64_t> want_sums;
    for (int64_t q = 0; q < n; ++q)
        for (int s = 0; s < 2; ++s) {
            const bool spot = q == 0 || q == n - 1 || q % TILE == 0 || q % TILE == TILE - 1 || q % 37 == phase;
            if (!spot) continue;
            const Key& k = ks[size_t((2 * q + s + phase) % int64_t(ks.size()))];
            for (int j = 0; j < K; ++j) tab[size_t(4 * j + 2 * s)][size_t(q)] = k.c[size_t(j)], tab[size_t(4 * j + 2 * s + 1)][size_t(q)] = k.m[size_t(j)];
            const int f = restated_fate(k, n_a, min_a, min_b, sums);
            if (f >= 0) ++want[4 * s + f];
            if (f == 0) {
                ++tested;
                want_sums.insert(want_sums.end(), sums, sums + 6);
            }
        }
    std::vector<std::unique_ptr<int32_t[]>> blocks;
    std::vector<const int32_t*> col[4];
    for (int j = 0; j < K; ++j)
        for (int f = 0; f < 4; ++f) {
            blocks.push_back(exact(tab[size_t(4 * j + f)]));
            col[f].push_back(blocks.back().get());
        }
    std::unique_ptr<const int32_t*[]> lists[4];
    for (int f = 0; f < 4; ++f) lists[f] = exact(col[f]);
    std::unique_ptr<int64_t[]> counters(new int64_t[8]), hist(new int64_t[20]), n_rec(new int64_t[1]);
    for (int j = 0; j < 20; ++j) hist[j] = 0;
    const size_t cap = size_t(tested);                                 // alpha 1: exactly every tested key
    std::unique_ptr<int32_t[]> pos(new int32_t[cap]), cA(new int32_t[cap]), mA(new int32_t[cap]), cB(new int32_t[cap]), mB(new int32_t[cap]);
    std::unique_ptr<uint8_t[]> strand(new uint8_t[cap]), nA(new uint8_t[cap]), nB(new uint8_t[cap]);
    std::unique_ptr<double[]> phi(new double[cap]), p(new double[cap]);
    const int rc = dm_diffrep_test_host(COV, alpha, min_a, min_b, n_a, n_b, n, lists[0].get(), lists[1].get(), lists[2].get(), lists[3].get(), counters.get(), hist.get(),
                                        int64_t(cap), pos.get(), strand.get(), cA.get(), mA.get(), cB.get(), mB.get(), nA.get(), nB.get(), phi.get(), p.get(), n_rec.get());
    CHECK(rc == DM_OK);
    for (int j = 0; j < 8; ++j) CHECK(counters[j] == want[j]);
    int64_t in_hist = 0;
    for (int j = 0; j < 20; ++j) in_hist += hist[j];
    CHECK(in_hist == tested);
    CHECK(n_rec[0] <= tested && (alpha < 1.0 || n_rec[0] == tested));
    for (int64_t i = 0; i < n_rec[0] && i < int64_t(cap); ++i) {
        CHECK(p[i] >= 0.0 && p[i] <= alpha && phi[i] >= 1.0);
        CHECK(i == 0 || 2 * int64_t(pos[i - 1]) + strand[i - 1] < 2 * int64_t(pos[i]) + strand[i]);          // key order
        CHECK(mA[i] >= 0 && mA[i] <= cA[i] && mB[i] >= 0 && mB[i] <= cB[i] && nA[i] >= min_a && nA[i] <= n_a && nB[i] >= min_b && nB[i] <= n_b);
        if (alpha >= 1.0) {
            const int64_t* w = &want_sums[size_t(6 * i)];
            CHECK(cA[i] == w[0] && mA[i] == w[1] && cB[i] == w[2] && mB[i] == w[3] && nA[i] == w[4] && nB[i] == w[5]);
        }
    }
}

bool close(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fabs(b); }

}  // namespace

int main() {
    const int shapes[4][4] = {{1, 2, 1, 2}, {2, 1, 2, 1}, {3, 5, 2, 4}, {8, 8, 8, 8}};                      // n_a, n_b, min_a, min_b
    for (const auto& sh : shapes)
        for (int64_t n : {int64_t(0), int64_t(1), int64_t(TILE - 1), int64_t(TILE), int64_t(TILE + 1), int64_t(3 * TILE + 5)})
            for (int phase : {0, 5}) {
                one_contig(sh[0], sh[1], sh[2], sh[3], n, phase, 1.0);
                one_contig(sh[0], sh[1], sh[2], sh[3], n, phase, 0.05);
            }
    // the F tail: closed forms
    const double pi = 3.14159265358979323846;
    for (double F : {1e-9, 0.01, 0.5, 0.99, 1.0, 1.01, 2.0, 4.0, 4.000001, 30.0, 1e3, 1.4e6}) {
        const double t1 = 1.0 - 2.0 / pi * std::atan(std::sqrt(F)), t2 = 1.0 - std::sqrt(F / (2.0 + F));
        const double s = std::sqrt(F / (4.0 + F)), t4 = 1.0 - s * (1.0 + 0.5 * (4.0 / (4.0 + F)));
        const double slack = F > 100.0 ? 1e-9 * F : 1e-12;            // (the closed forms themselves cancel in the far tail)
        CHECK(close(dfr::f_tail(1, F), t1, slack) && close(dfr::f_tail(2, F), t2, slack) && close(dfr::f_tail(4, F), t4, slack * (F > 100.0 ? F : 1.0)));
    }
    for (int nu = 1; nu <= 14; ++nu) {
        CHECK(dfr::f_tail(nu, 0.0) == 1.0);
        double before = 1.0;
        for (double F = 0.125; F < 4e6; F *= 2.0) {                    // decreasing in F, within (0, 1), across the reflection at x = 1/2
            const double p = dfr::f_tail(nu, F);
            CHECK(p > 0.0 && p < before);
            before = p;
        }
    }
    // the refusals: nothing is read
    int64_t counters[8], hist[20] = {}, n_rec = -1;
    const int32_t z[1] = {0};
    const int32_t* const zz[16] = {z, z, z, z, z, z, z, z, z, z, z, z, z, z, z, z};
    const int32_t* const hole[3] = {z, nullptr, z};
#define RUN(cov, alpha, ma, mb, na, nb, len, a, b, c, d, cap) \
    dm_diffrep_test_host(cov, alpha, ma, mb, na, nb, len, a, b, c, d, counters, hist, cap, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n_rec)
    CHECK(RUN(0, 0.05, 1, 2, 1, 2, 1, zz, zz, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.0, 1, 2, 1, 2, 1, zz, zz, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 1.5, 1, 2, 1, 2, 1, zz, zz, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.05, 1, 1, 1, 2, 1, zz, zz, zz, zz, 0) == DM_EINVAL);                                    // a + b < 3
    CHECK(RUN(5, 0.05, 1, 1, 1, 1, 1, zz, zz, zz, zz, 0) == DM_EINVAL);                                    // two replicates
    CHECK(RUN(5, 0.05, 0, 3, 1, 3, 1, zz, zz, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.05, 2, 2, 1, 2, 1, zz, zz, zz, zz, 0) == DM_EINVAL);                                    // a > n_a
    CHECK(RUN(5, 0.05, 1, 2, 9, 2, 1, zz, zz, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.05, 1, 2, 1, 0, 1, zz, zz, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.05, 1, 2, 1, 2, -1, zz, zz, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.05, 1, 2, 1, 2, 1, zz, nullptr, zz, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.05, 1, 2, 1, 2, 1, zz, zz, hole, zz, 0) == DM_EINVAL);
    CHECK(RUN(5, 0.05, 1, 2, 1, 2, 1, zz, zz, zz, zz, 1) == DM_EINVAL);                                    // records wanted, no arrays
    CHECK(n_rec == -1);
    CHECK(RUN(5, 0.05, 1, 2, 1, 2, 0, hole, hole, hole, hole, 0) == DM_OK);                                // an empty contig: no table is read
    CHECK(n_rec == 0 && counters[0] == 0 && hist[19] == 0);
    CHECK(dm_diffrep_max_replicates() == 8);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("DIFFREP-DRIVER-OK\n");
    return 0;
}
