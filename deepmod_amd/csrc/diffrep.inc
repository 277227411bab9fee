// diffrep.inc — `diffmod --replicates 1`: the fate of a key over replicates, the quasi-binomial F test of one key, the compiled host twin, and (under
// hipcc) the handle and the C ABI.  The first part is plain C++: part of offline.hip, and compiled by g++ as it stands (tests/diffrep_driver.cpp).  The
// kernel of diffrep.hip.inc and dm_diffrep_test_host run the same routine per key (dfr::test_key), so the device and the host differ only in their
// log, sqrt and division.  deepmod_amd/diffmod.py (RepHostEngine) states the semantics in integers and 50-digit decimals; DESIGN.md 22.
//
// One contig: n_a sample and n_b control replicates (1..8 each, 3 or more together), each a '+' and a '-' table (coverage, modified count per
// position).  A key is (strand, position).  A modified count is first held to 0..coverage (a coverage below 0 counts as 0); replicate i is used at the
// key iff c_i >= cov; nA, nB are the used replicates of either group, C_g and M_g the sums of c and m over them.  The first rule that applies decides:
//   1  every c_i == 0: ignored        2  nA < min_a: shallow_sample        3  nB < min_b: shallow_control
//   4  C_A + C_B > MAX_TOTAL (in 64 bits): too_deep        5  tested
// A tested key: nu = nA + nB - 2, C = C_A + C_B, M = M_A + M_B.  M_A C_B == M_B C_A in integers: p = 1, phi = 1.  Else
//   h(M, C) = M ln(M / C) + (C - M) ln((C - M) / C)   (a term whose factor is 0 is 0),      D = max(0, 2 [h(M_A, C_A) + h(M_B, C_B) - h(M, C)]),
//   X2 = sum over the groups with 0 < M_g < C_g, over their used replicates in slot order, of r_i^2 / (c_i M_g (C_g - M_g)),  r_i = m_i C_g - c_i M_g,
//   phi = max(1, X2 / nu),  F = D / phi,  p = I_x(nu / 2, 1 / 2) at x = nu / (nu + F): the upper tail of F(1, nu).
// The incomplete beta (dfr::f_tail), with y = F / (nu + F) formed by its own division and K[nu] = 1 / ((nu / 2) B(nu / 2, 1 / 2)):
//   x <= 1/2:  p = x^(nu/2) y^(1/2) K[nu] S(nu/2 + 1/2, nu/2 + 1; x)           S(a, b; z) = sum over n >= 0 of z^n (a)_n / (b)_n
//   x >  1/2:  p = 1 - x^(nu/2) y^(1/2) nu K[nu] S(nu/2 + 1/2, 3/2; y)         (the reflection I_x(a, 1/2) = 1 - I_y(1/2, a))
// x^(nu/2) is sqrt(x) multiplied nu times; S is summed from n = 0 up and ends behind the first term at most 2^-56 of the sum so far, which depends on
// nu and F alone: fewer than 90 terms for z <= 1/2.  No pow, no exp, no table in memory.
// Two guarded parts, so that this file and diffrep.hip.inc can be included in either order: the rule, which the kernel includes, and the handle,
// which includes the kernel.
#ifndef DM_DIFFREP_RULE_INC
#define DM_DIFFREP_RULE_INC
#ifdef DM_DIFFMOD_RULE_ONLY                         // the fates, the histogram bins and `held` are diffmod's: its rule part alone
#include "diffmod.inc"
#else
#define DM_DIFFMOD_RULE_ONLY
#include "diffmod.inc"
#undef DM_DIFFMOD_RULE_ONLY
#endif

namespace dfr {

using dfk::F_IGNORED;
using dfk::F_SHALLOW_CONTROL;
using dfk::F_SHALLOW_SAMPLE;
using dfk::F_TESTED;
using dfk::F_TOO_DEEP;
using dfk::HIST_BINS;
using dfk::MAX_LENGTH;
using dfk::MAX_TOTAL;
using dfk::N_COUNT;

constexpr int MAX_REPS = 8;                         // replicates of a group at most (dm_diffrep_max_replicates)
constexpr int SLOTS = 2 * MAX_REPS;                 // slot i < MAX_REPS: sample replicate i; slot MAX_REPS + j: control replicate j
constexpr int MAX_TERMS = 128;                      // of a series; never reached (fewer than 90 are summed for z <= 1/2)
constexpr double STOP = 0x1p-56;                    // a series ends behind the first term at most this share of its sum

struct Rule {
    int cov, min_a, min_b, n_a, n_b;
    double alpha;
};

// what create can check: null, or what is wrong
inline const char* check_options(const int cov, const double alpha, const int min_a, const int min_b) {
    if (const char* why = dfk::check_rule(cov, alpha)) return why;
    if (min_a < 1 || min_a > MAX_REPS || min_b < 1 || min_b > MAX_REPS) return "least replicate counts of 1 to 8 each";
    if (min_a + min_b < 3) return "least replicate counts of 3 or more together";
    return nullptr;
}

// and what a run can: the replicate counts against the least counts
inline const char* check_rule(const Rule& r) {
    if (const char* why = check_options(r.cov, r.alpha, r.min_a, r.min_b)) return why;
    if (r.n_a < 1 || r.n_a > MAX_REPS || r.n_b < 1 || r.n_b > MAX_REPS) return "1 to 8 replicates of either group";
    if (r.n_a + r.n_b < 3) return "3 or more replicates together";
    if (r.min_a > r.n_a || r.min_b > r.n_b) return "least replicate counts of at most the replicates of either group";
    return nullptr;
}

struct Tested {
    int cA, mA, cB, mB, nA, nB;                     // the sums over the used replicates and their numbers
    double phi, p;
};

// 1 / ((nu / 2) B(nu / 2, 1 / 2)), nu = 1 .. 14: rationals for even nu, rationals over pi for odd nu, rounded once
BED_HD inline double beta_front(const int nu) {
    switch (nu) {
        case 1: return 0.63661977236758134308;
        case 2: return 0.5;
        case 3: return 0.42441318157838756205;
        case 4: return 0.375;
        case 5: return 0.33953054526271004964;
        case 6: return 0.3125;
        case 7: return 0.29102618165375147112;
        case 8: return 0.2734375;
        case 9: return 0.25868993924777908544;
        case 10: return 0.24609375;
        case 11: return 0.23517267204343553222;
        case 12: return 0.2255859375;
        case 13: return 0.21708246650163279897;
        default: return 0.20947265625;
    }
}

// S(a, b; z) = sum of z^n (a)_n / (b)_n, 0 <= z <= 1/2, a and b positive
BED_HD inline double series(const double a, const double b, const double z) {
    double t = 1.0, s = 1.0;
    for (int n = 0; n < MAX_TERMS; ++n) {
        t = (t * z) * ((a + n) / (b + n));
        s += t;
        if (t <= STOP * s) break;
    }
    return s;
}

// the upper tail of F(1, nu) at F >= 0, nu = 1 .. 14
BED_HD inline double f_tail(const int nu, const double F) {
    const double den = double(nu) + F, x = double(nu) / den, y = F / den, a = 0.5 * nu;
    const double rx = ::sqrt(x);
    double front = ::sqrt(y) * beta_front(nu);
    for (int k = 0; k < nu; ++k) front *= rx;
    if (x <= 0.5) return front * series(a + 0.5, a + 1.0, x);
    const double p = 1.0 - (front * double(nu)) * series(a + 0.5, 1.5, y);
    return p < 0.0 ? 0.0 : p;
}

BED_HD inline double h_of(const long long M, const long long C) {
    double v = 0.0;
    if (M > 0) v += double(M) * ::log(double(M) / double(C));
    if (C - M > 0) v += double(C - M) * ::log(double(C - M) / double(C));
    return v;
}

// The fate of a key (F_*) from the counts of its SLOTS slots as the tables hold them (a slot without a replicate: 0, 0); t is set for a tested key.
BED_HD inline int test_key(const Rule& r, const int (&c_in)[SLOTS], const int (&m_in)[SLOTS], Tested& t) {
    int c[SLOTS], m[SLOTS];
    long long C[2] = {0, 0}, M[2] = {0, 0};
    int n[2] = {0, 0};
    bool any = false;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int cv = c_in[i] > 0 ? c_in[i] : 0;
        any = any || cv > 0;
        const bool used = cv >= r.cov;
        c[i] = used ? cv : 0;                       // (cov >= 1: an unused slot is one of coverage 0 from here on)
        m[i] = used ? dfk::held(m_in[i], cv) : 0;
        const int g = i < MAX_REPS ? 0 : 1;
        C[g] += c[i];
        M[g] += m[i];
        n[g] += used ? 1 : 0;
    }
    if (!any) return F_IGNORED;
    if (n[0] < r.min_a) return F_SHALLOW_SAMPLE;
    if (n[1] < r.min_b) return F_SHALLOW_CONTROL;
    if (C[0] + C[1] > MAX_TOTAL) return F_TOO_DEEP;
    t.cA = int(C[0]), t.mA = int(M[0]), t.cB = int(C[1]), t.mB = int(M[1]), t.nA = n[0], t.nB = n[1];
    if (M[0] * C[1] == M[1] * C[0]) {
        t.phi = 1.0, t.p = 1.0;
        return F_TESTED;
    }
    const int nu = n[0] + n[1] - 2;
    const double D2 = (h_of(M[0], C[0]) + h_of(M[1], C[1])) - h_of(M[0] + M[1], C[0] + C[1]);
    const double D = D2 > 0.0 ? 2.0 * D2 : 0.0;
    double X2 = 0.0;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int g = i < MAX_REPS ? 0 : 1;
        const long long spread = M[g] * (C[g] - M[g]);                // < 2^38
        if (c[i] > 0 && spread > 0) {
            const double ri = double((long long)m[i] * C[g] - (long long)c[i] * M[g]);      // exact: below 2^41 in size
            X2 += (ri * ri) / double((long long)c[i] * spread);
        }
    }
    const double scaled = X2 / double(nu);
    t.phi = scaled > 1.0 ? scaled : 1.0;
    const double p = f_tail(nu, D / t.phi);
    t.p = p < 1.0 ? p : 1.0;
    return F_TESTED;
}

}  // namespace dfr

#ifdef __HIP__
#define DFR_FAIL(...) fail(DM_EINVAL, __VA_ARGS__)
#else
#define DFR_FAIL(...) DM_EINVAL
#endif

extern "C" int dm_diffrep_max_replicates(void) { return dfr::MAX_REPS; }

// The compiled host twin of one run (no GPU needed): a contig of len >= 0 positions; cov_plus, mod_plus, cov_minus, mod_minus are n_a + n_b pointers
// each, sample replicates first, to tables of len entries.  counters [2][4] are set, hist [20] is added to, *n_records = the tested keys with
// p <= alpha, of which the first `cap` are written to the ten record arrays (key order); the arrays may be null when cap is 0.
extern "C" int dm_diffrep_test_host(int cov, double alpha, int min_a, int min_b, int n_a, int n_b, int64_t len, const int32_t* const* cov_plus, const int32_t* const* mod_plus,
                                    const int32_t* const* cov_minus, const int32_t* const* mod_minus, int64_t* counters, int64_t* hist, int64_t cap, int32_t* pos,
                                    uint8_t* strand, int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, uint8_t* nA, uint8_t* nB, double* phi, double* p, int64_t* n_records) {
    const dfr::Rule rule = {cov, min_a, min_b, n_a, n_b, alpha};
    if (const char* why = dfr::check_rule(rule)) return DFR_FAIL("dm_diffrep_test_host: %s", why);
    if (len < 0 || len > dfr::MAX_LENGTH) return DFR_FAIL("dm_diffrep_test_host: a contig of %lld positions (0 to 2^31 - 1)", (long long)len);
    if (!counters || !hist || !n_records || cap < 0 || !cov_plus || !mod_plus || !cov_minus || !mod_minus) return DFR_FAIL("dm_diffrep_test_host: null argument");
    if (len > 0)
        for (int j = 0; j < n_a + n_b; ++j)
            if (!cov_plus[j] || !mod_plus[j] || !cov_minus[j] || !mod_minus[j]) return DFR_FAIL("dm_diffrep_test_host: replicate %d has a null table", j);
    if (cap > 0 && (!pos || !strand || !cA || !mA || !cB || !mB || !nA || !nB || !phi || !p)) return DFR_FAIL("dm_diffrep_test_host: null record array");
    const int32_t* const* const tab[2][2] = {{cov_plus, mod_plus}, {cov_minus, mod_minus}};
    for (int j = 0; j < 2 * dfr::N_COUNT; ++j) counters[j] = 0;
    int64_t n = 0;
    for (int64_t q = 0; q < len; ++q)
        for (int s = 0; s < 2; ++s) {
            int c[dfr::SLOTS] = {}, m[dfr::SLOTS] = {};
            for (int j = 0; j < n_a + n_b; ++j) {
                const int slot = j < n_a ? j : dfr::MAX_REPS + j - n_a;
                c[slot] = tab[s][0][j][q];
                m[slot] = tab[s][1][j][q];
            }
            dfr::Tested t;
            const int f = dfr::test_key(rule, c, m, t);
            if (f == dfr::F_IGNORED) continue;
            ++counters[s * dfr::N_COUNT + f];
            if (f != dfr::F_TESTED) continue;
            ++hist[dfk::bin_of(t.p)];
            if (!(t.p <= alpha)) continue;
            if (n < cap) {
                pos[n] = int32_t(q);
                strand[n] = uint8_t(s);
                cA[n] = t.cA, mA[n] = t.mA, cB[n] = t.cB, mB[n] = t.mB;
                nA[n] = uint8_t(t.nA), nB[n] = uint8_t(t.nB);
                phi[n] = t.phi;
                p[n] = t.p;
            }
            ++n;
        }
    *n_records = n;
    return DM_OK;
}

#endif  // DM_DIFFREP_RULE_INC

#if defined(__HIP__) && !defined(DM_DIFFREP_HANDLE_INC) && !defined(DM_DIFFREP_RULE_ONLY)
#define DM_DIFFREP_HANDLE_INC
#include "diffrep.hip.inc"
#include "tablestage.hip.inc"

struct dm_diffrep_buf {
    // HIST [20]; COUNTS: the counters [2][4], then n_records; TILE_N / TILE_OFF: records per tile and their scan; the records: R_POS .. R_P
    enum { HIST, COUNTS, TILE_N, TILE_OFF, R_POS, R_STRAND, R_CA, R_MA, R_CB, R_MB, R_NA, R_NB, R_PHI, R_P, N_BUF };
};
struct dm_diffrep : dm_diffrep_buf, TableStage<4, dm_diffrep_buf::N_BUF> {    // events: the count pass with its scan, the write pass: begin / end each
    int cov = 0, min_a = 0, min_b = 0;
    double alpha = 0.0;
    long long n_records = 0;                        // of the last run
    double count_ms = 0.0, write_ms = 0.0;
};

extern "C" {

void dm_diffrep_destroy(dm_diffrep* h) {
    if (!h) return;
    h->shut();
    delete h;
}

dm_diffrep* dm_diffrep_create(int device, int cov, double alpha, int min_a, int min_b) {
    if (const char* why = dfr::check_options(cov, alpha, min_a, min_b)) {
        fail(DM_EINVAL, "dm_diffrep_create: %s (got cov %d alpha %g least counts %d, %d)", why, cov, alpha, min_a, min_b);
        return nullptr;
    }
    if (!table_stage_device("dm_diffrep", device)) return nullptr;
    using B = dm_diffrep;
    dm_diffrep* h = new dm_diffrep;
    h->cov = cov, h->alpha = alpha, h->min_a = min_a, h->min_b = min_b;
    bool ok = h->open(device, "dm_diffrep");
    ok = ok && h->b.ensure(B::HIST, dfr::HIST_BINS * 8) == DM_OK && h->b.ensure(B::COUNTS, dfr::N_WORDS * 8) == DM_OK;
    ok = ok && h->zero_block(B::HIST, dfr::HIST_BINS * 8) == DM_OK;
    if (!ok) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_diffrep_create: stream, events or counters on device %d", device);
        dm_diffrep_destroy(h);
        return nullptr;
    }
    return h;
}

int dm_diffrep_run(dm_diffrep* h, int n_a, int n_b, dm_summary* const* plus, dm_summary* const* minus, int64_t* counters, int64_t* n_records) {
    using B = dm_diffrep;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!counters || !n_records || !plus || !minus) return fail(DM_EINVAL, "dm_diffrep_run: null argument");
    const dfr::Rule rule = {h->cov, h->min_a, h->min_b, n_a, n_b, h->alpha};
    if (const char* why = dfr::check_rule(rule)) return fail(DM_EINVAL, "dm_diffrep_run: %s (got %d and %d replicates, least counts %d, %d)", why, n_a, n_b, h->min_a, h->min_b);
    const int reps = n_a + n_b;
    dm_summary* tab[2 * dfr::SLOTS];                                  // replicate j: its '+' table at 2 j, its '-' table at 2 j + 1
    for (int j = 0; j < reps; ++j) {
        tab[2 * j] = plus[j], tab[2 * j + 1] = minus[j];
        if (!plus[j] || !minus[j]) return fail(DM_EINVAL, "dm_diffrep_run: replicate %d: two tables, one per strand (null handle)", j);
    }
    for (int j = 0; j < 2 * reps; ++j)
        for (int k = 0; k < j; ++k)
            if (tab[j] == tab[k]) return fail(DM_EINVAL, "dm_diffrep_run: the same table twice (replicate %d and replicate %d): every replicate has two tables of its own", k / 2, j / 2);
    const long long len = dm_summary_length(tab[0]);
    if (len < 1 || len > dfr::MAX_LENGTH) return fail(DM_EINVAL, "dm_diffrep_run: tables of %lld positions (1 to 2^31 - 1)", len);
    for (int j = 0; j < 2 * reps; ++j)
        if (dm_summary_length(tab[j]) != len)
            return fail(DM_EINVAL, "dm_diffrep_run: tables of different lengths: table %d has %lld positions, table 0 %lld", j, (long long)dm_summary_length(tab[j]), len);
    int rc;
    if ((rc = h->tables_ready("dm_diffrep_run", tab, 2 * reps)) != DM_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    h->n_records = 0;
    const long long tiles = (len + dfr::TILE_POS - 1) / dfr::TILE_POS;
    if ((rc = h->b.ensure(B::TILE_N, size_t(tiles) * 4)) != DM_OK || (rc = h->b.ensure(B::TILE_OFF, size_t(tiles) * 8)) != DM_OK) return rc;
    hipStream_t s = h->stream;
    dfr::Tables t = {};
    for (int j = 0; j < reps; ++j) {
        const int slot = j < n_a ? j : dfr::MAX_REPS + j - n_a;
        t.t[0][slot] = static_cast<const int*>(dm_summary_device_ptr(tab[2 * j]));
        t.t[1][slot] = static_cast<const int*>(dm_summary_device_ptr(tab[2 * j + 1]));
    }
    unsigned long long* d_counts = h->b.ptr<unsigned long long>(B::COUNTS);
    unsigned long long* d_hist = h->b.ptr<unsigned long long>(B::HIST);
    const dim3 grid{unsigned(std::min<long long>(tiles, dfr::MAX_BLOCKS))}, block{dfr::THREADS};
    const dfr::Records none = {};
    // 1  the fates and the tests: counters, the histogram, records per tile; their scan
    HIP_TRY(hipMemsetAsync(d_counts, 0, dfr::N_WORDS * 8, s));
    HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(dfr::sweep_kernel<false>, grid, block, 0, s, len, t, rule, h->b.ptr<int>(B::TILE_N), h->b.ptr<const long long>(B::TILE_OFF), none, d_counts, d_hist);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dfk::scan_kernel, dim3(1), block, 0, s, h->b.ptr<const int>(B::TILE_N), tiles, h->b.ptr<long long>(B::TILE_OFF), d_counts + dfr::W_RECORDS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[1], s));
    long long got[dfr::N_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(got, d_counts, sizeof got, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = add_time(h->ev[0], h->ev[1], h->count_ms)) != DM_OK) return rc;
    for (int j = 0; j < 2 * dfr::N_COUNT; ++j) counters[j] = got[j];
    const long long n_rec = got[dfr::W_RECORDS];
    *n_records = 0;
    if (n_rec == 0) return DM_OK;
    // 2  the records in key order
    for (int which : {int(B::R_POS), int(B::R_CA), int(B::R_MA), int(B::R_CB), int(B::R_MB)})
        if ((rc = h->b.ensure(which, size_t(n_rec) * 4)) != DM_OK) return rc;
    for (int which : {int(B::R_STRAND), int(B::R_NA), int(B::R_NB)})
        if ((rc = h->b.ensure(which, size_t(n_rec))) != DM_OK) return rc;
    if ((rc = h->b.ensure(B::R_PHI, size_t(n_rec) * 8)) != DM_OK || (rc = h->b.ensure(B::R_P, size_t(n_rec) * 8)) != DM_OK) return rc;
    const dfr::Records r = {h->b.ptr<int>(B::R_POS), h->b.ptr<unsigned char>(B::R_STRAND), h->b.ptr<int>(B::R_CA), h->b.ptr<int>(B::R_MA), h->b.ptr<int>(B::R_CB),
                            h->b.ptr<int>(B::R_MB), h->b.ptr<unsigned char>(B::R_NA), h->b.ptr<unsigned char>(B::R_NB), h->b.ptr<double>(B::R_PHI), h->b.ptr<double>(B::R_P),
                            n_rec};
    HIP_TRY(hipEventRecord(h->ev[2], s));
    hipLaunchKernelGGL(dfr::sweep_kernel<true>, grid, block, 0, s, len, t, rule, h->b.ptr<int>(B::TILE_N), h->b.ptr<const long long>(B::TILE_OFF), r, d_counts, d_hist);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = add_time(h->ev[2], h->ev[3], h->write_ms)) != DM_OK) return rc;
    h->n_records = n_rec;
    *n_records = n_rec;
    return DM_OK;
}

int dm_diffrep_fetch_records(dm_diffrep* h, int64_t first, int64_t count, int32_t* pos, uint8_t* strand, int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, uint8_t* nA,
                             uint8_t* nB, double* phi, double* p) {
    using B = dm_diffrep;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (first < 0 || count < 0 || first + count > h->n_records)
        return fail(DM_EINVAL, "dm_diffrep_fetch_records: records %lld .. %lld of %lld", (long long)first, (long long)(first + count), h->n_records);
    if (count == 0) return DM_OK;
    if (!pos || !strand || !cA || !mA || !cB || !mB || !nA || !nB || !phi || !p) return fail(DM_EINVAL, "dm_diffrep_fetch_records: null argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t n = size_t(count), f = size_t(first);
    HIP_TRY(hipMemcpyAsync(pos, h->b.ptr<int>(B::R_POS) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(strand, h->b.ptr<unsigned char>(B::R_STRAND) + f, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cA, h->b.ptr<int>(B::R_CA) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(mA, h->b.ptr<int>(B::R_MA) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cB, h->b.ptr<int>(B::R_CB) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(mB, h->b.ptr<int>(B::R_MB) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nA, h->b.ptr<unsigned char>(B::R_NA) + f, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nB, h->b.ptr<unsigned char>(B::R_NB) + f, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(phi, h->b.ptr<double>(B::R_PHI) + f, n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p, h->b.ptr<double>(B::R_P) + f, n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

int dm_diffrep_fetch_hist(dm_diffrep* h, int64_t* hist) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!hist) return fail(DM_EINVAL, "dm_diffrep_fetch_hist: null argument");
    return h->fetch_block(dm_diffrep::HIST, hist, dfr::HIST_BINS * 8);
}

int dm_diffrep_reset(dm_diffrep* h) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->n_records = 0;
    return h->zero_block(dm_diffrep::HIST, dfr::HIST_BINS * 8);
}

int dm_diffrep_times(dm_diffrep* h, double* count_ms, double* write_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (count_ms) *count_ms = h->count_ms;
    if (write_ms) *write_ms = h->write_ms;
    return DM_OK;
}

}  // extern "C"
#endif  // the handle
