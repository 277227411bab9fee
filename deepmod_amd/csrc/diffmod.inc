// diffmod.inc — `diffmod`: the fate of a key, Fisher's exact test of one key, the compiled host twin, and (under hipcc) the handle and the C ABI.
// The first part is plain C++: part of offline.hip, and compiled by g++ as it stands (tests/diffmod_driver.cpp).  The kernels of diffmod.hip.inc and
// dm_diffmod_test_host run the same routines (dfk::fate, dfk::support, dfk::log_term) on the same table (dfk::lf_table), so the device and the host
// differ only in the order a key's terms are summed in.  deepmod_amd/diffmod.py (HostEngine) states the semantics with exact integers; DESIGN.md 21.
//
// One contig: the sample's '+' and '-' tables (coverage, modified count per position) and the pooled controls' tables.  Each key (strand s,
// position p) has cA, mA of the sample and cB, mB of the controls; the first rule that applies decides (dfk::fate):
//   1  cA == 0 and cB == 0: ignored        2  cA < cov: shallow_sample        3  cB < cov: shallow_control
//   4  cA + cB > MAX_TOTAL: too_deep       5  tested
// A tested key: n1 = cA, n2 = cB, M = mA + mB, N = n1 + n2; the support is x in [max(0, M - n2), min(n1, M)], S tables;
//   L(x) = lf[n1] + lf[n2] + lf[M] + lf[N-M] - lf[N] - lf[x] - lf[n1-x] - lf[M-x] - lf[n2-M+x],      lf[k] = lgamma(k + 1)
// and p = min(1, sum of exp(L(x)) over the x with L(x) <= L(mA) + 1e-7): the two-sided rule of R's fisher.test, decided in the log domain.  S == 1
// (M == 0 or M == N among others) is p = 1 without a table read.  A modified count is held to 0..coverage before anything else, so no index can leave
// lf whatever the tables hold (the tables of merge never hold such a count).
// Two guarded parts, so that this file and diffmod.hip.inc can be included in either order: the rule, which the kernels include, and the handle,
// which includes the kernels.
#ifndef DM_DIFFMOD_RULE_INC
#define DM_DIFFMOD_RULE_INC
#ifdef __HIP__
#include "host.h"
#endif
#include <cmath>
#include <vector>
#include "bedline.inc"
#include "../../include/deepmod_hip.h"

namespace dfk {

constexpr long long MAX_LENGTH = 0x7fffffffLL;      // positions of a contig, 1 to 2^31 - 1
constexpr int MAX_TOTAL = 1 << 20;                  // cA + cB of a tested key at most: lf has MAX_TOTAL + 1 entries (dm_diffmod_max_total)
constexpr int HIST_BINS = 20;                       // the p histogram: bin = min(19, int(20 p))
constexpr double TIE = 1e-7;                        // a table as probable as the observed one, to this much in the log domain, counts
enum { K_TESTED, K_SHALLOW_SAMPLE, K_SHALLOW_CONTROL, K_TOO_DEEP, N_COUNT };    // the counters of a strand
enum { F_IGNORED = -1, F_TESTED = K_TESTED, F_SHALLOW_SAMPLE = K_SHALLOW_SAMPLE, F_SHALLOW_CONTROL = K_SHALLOW_CONTROL, F_TOO_DEEP = K_TOO_DEEP };

// null: the options are in range; else what is wrong with them
inline const char* check_rule(const int cov, const double alpha) {
    if (cov < 1) return "a least coverage of 1 or more";
    if (!(alpha > 0.0 && alpha <= 1.0)) return "an alpha above 0 and at most 1";
    return nullptr;
}

BED_HD inline int held(const int m, const int c) { return m < 0 ? 0 : (m > c ? c : m); }

// The fate of a key: F_*
BED_HD inline int fate(const int cov, const int cA, const int cB) {
    if (cA <= 0 && cB <= 0) return F_IGNORED;
    if (cA < cov) return F_SHALLOW_SAMPLE;
    if (cB < cov) return F_SHALLOW_CONTROL;
    if ((long long)cA + cB > MAX_TOTAL) return F_TOO_DEEP;
    return F_TESTED;
}

// The support of a tested key (modified counts held to 0..coverage): lo = the smallest x; -> S = the number of tables, 1 or more
BED_HD inline int support(const int cA, const int mA, const int cB, const int mB, int& lo) {
    const int M = mA + mB;
    lo = M - cB > 0 ? M - cB : 0;
    return (cA < M ? cA : M) - lo + 1;
}

// L(x) of the key, summed in the order stated above.  Every index is in [0, N], N <= MAX_TOTAL, for lo <= x <= lo + S - 1.
BED_HD inline double log_term(const double* lf, const int n1, const int n2, const int M, const int x) {
    const int N = n1 + n2;
    return lf[n1] + lf[n2] + lf[M] + lf[N - M] - lf[N] - lf[x] - lf[n1 - x] - lf[M - x] - lf[n2 - M + x];
}

// the probability of table x if it counts (cut = L(observed) + TIE), else 0
BED_HD inline double term(const double* lf, const int n1, const int n2, const int M, const int x, const double cut) {
    const double L = log_term(lf, n1, n2, M, x);
    return L <= cut ? ::exp(L) : 0.0;
}

BED_HD inline double capped(const double sum) { return sum < 1.0 ? sum : 1.0; }

BED_HD inline int bin_of(const double p) {
    const int b = int(p * HIST_BINS);
    return b > HIST_BINS - 1 ? HIST_BINS - 1 : b;
}

// p of a tested key, the terms summed from the smallest x up
BED_HD inline double fisher_p(const double* lf, const int cA, const int mA_, const int cB, const int mB_) {
    const int mA = held(mA_, cA), mB = held(mB_, cB);
    int lo;
    const int S = support(cA, mA, cB, mB, lo);
    if (S == 1) return 1.0;
    const int M = mA + mB;
    const double cut = log_term(lf, cA, cB, M, mA) + TIE;
    double sum = 0.0;
    for (int x = lo; x < lo + S; ++x) sum += term(lf, cA, cB, M, x, cut);
    return capped(sum);
}

// lf[k] = lgamma(k + 1), k = 0 .. MAX_TOTAL: computed once per process; the device holds a copy of exactly these doubles
inline const double* lf_table() {
    static const std::vector<double> table = [] {
        std::vector<double> t(size_t(MAX_TOTAL) + 1);
        for (int k = 0; k <= MAX_TOTAL; ++k) t[size_t(k)] = std::lgamma(double(k) + 1.0);
        return t;
    }();
    return table.data();
}

}  // namespace dfk

#ifdef __HIP__
#define DFK_FAIL(...) fail(DM_EINVAL, __VA_ARGS__)
#else
#define DFK_FAIL(...) DM_EINVAL
#endif

extern "C" int dm_diffmod_max_total(void) { return dfk::MAX_TOTAL; }

// The compiled host twin of one run (no GPU needed): a contig of len >= 0 positions, the eight tables of len entries each.  counters [2][4] are set,
// hist [20] is added to, *n_records = the tested keys with p <= alpha, of which the first `cap` are written to the seven record arrays (key order:
// ascending position, '+' before '-'); the arrays may be null when cap is 0.
extern "C" int dm_diffmod_test_host(int cov, double alpha, int64_t len, const int32_t* cov_plus, const int32_t* mod_plus, const int32_t* cov_minus, const int32_t* mod_minus,
                                    const int32_t* ctrl_cov_plus, const int32_t* ctrl_mod_plus, const int32_t* ctrl_cov_minus, const int32_t* ctrl_mod_minus,
                                    int64_t* counters, int64_t* hist, int64_t cap, int32_t* pos, uint8_t* strand, int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, double* p,
                                    int64_t* n_records) {
    const char* why = dfk::check_rule(cov, alpha);
    if (why) return DFK_FAIL("dm_diffmod_test_host: %s", why);
    if (len < 0 || len > dfk::MAX_LENGTH) return DFK_FAIL("dm_diffmod_test_host: a contig of %lld positions (0 to 2^31 - 1)", (long long)len);
    if (!ctrl_cov_plus || !ctrl_mod_plus || !ctrl_cov_minus || !ctrl_mod_minus) {
        if (len > 0 || ctrl_cov_plus || ctrl_mod_plus || ctrl_cov_minus || ctrl_mod_minus) return DFK_FAIL("dm_diffmod_test_host: the controls are missing (four tables)");
    }
    if (!counters || !hist || !n_records || cap < 0 || (len > 0 && (!cov_plus || !mod_plus || !cov_minus || !mod_minus))) return DFK_FAIL("dm_diffmod_test_host: null argument");
    if (cap > 0 && (!pos || !strand || !cA || !mA || !cB || !mB || !p)) return DFK_FAIL("dm_diffmod_test_host: null record array");
    const int32_t* const tab[2][4] = {{cov_plus, mod_plus, ctrl_cov_plus, ctrl_mod_plus}, {cov_minus, mod_minus, ctrl_cov_minus, ctrl_mod_minus}};
    for (int j = 0; j < 2 * dfk::N_COUNT; ++j) counters[j] = 0;
    const double* lf = dfk::lf_table();
    int64_t n = 0;
    for (int64_t q = 0; q < len; ++q)
        for (int s = 0; s < 2; ++s) {
            const int a = tab[s][0][q], b = tab[s][2][q];
            const int f = dfk::fate(cov, a, b);
            if (f == dfk::F_IGNORED) continue;
            ++counters[s * dfk::N_COUNT + f];
            if (f != dfk::F_TESTED) continue;
            const int ma = dfk::held(tab[s][1][q], a), mb = dfk::held(tab[s][3][q], b);
            const double pv = dfk::fisher_p(lf, a, ma, b, mb);
            ++hist[dfk::bin_of(pv)];
            if (!(pv <= alpha)) continue;
            if (n < cap) {
                pos[n] = int32_t(q);
                strand[n] = uint8_t(s);
                cA[n] = a;
                mA[n] = ma;
                cB[n] = b;
                mB[n] = mb;
                p[n] = pv;
            }
            ++n;
        }
    *n_records = n;
    return DM_OK;
}

#endif  // DM_DIFFMOD_RULE_INC

#if defined(__HIP__) && !defined(DM_DIFFMOD_HANDLE_INC) && !defined(DM_DIFFMOD_RULE_ONLY)
#define DM_DIFFMOD_HANDLE_INC
#include "diffmod.hip.inc"
#include "tablestage.hip.inc"

struct dm_diffmod_buf {
    // LF: the table; HIST [20]; COUNTS: the counters [2][4], then n_work, n_large, n_records; TILE_N / TILE_OFF: tested keys per tile and their scan;
    // the work list: KEY (2 pos + strand), CA, MA, CB, MB, P; LARGE: indices of the keys above SMALL_S; CHUNK_N / CHUNK_OFF: records per chunk of the
    // work list and their scan; the records: R_POS .. R_P
    enum { LF, HIST, COUNTS, TILE_N, TILE_OFF, KEY, CA, MA, CB, MB, P, LARGE, CHUNK_N, CHUNK_OFF, R_POS, R_STRAND, R_CA, R_MA, R_CB, R_MB, R_P, N_BUF };
};
struct dm_diffmod : dm_diffmod_buf, TableStage<6, dm_diffmod_buf::N_BUF> {    // events: select: count pass, write pass; fisher: begin / end each
    int cov = 0;
    double alpha = 0.0;
    long long n_records = 0;                        // of the last run
    double select_ms = 0.0, fisher_ms = 0.0;
};

extern "C" {

int dm_diffmod_tile_positions(void) { return dfk::TILE_POS; }
int dm_diffmod_small_support(void) { return dfk::SMALL_S; }

void dm_diffmod_destroy(dm_diffmod* h) {
    if (!h) return;
    h->shut();
    delete h;
}

dm_diffmod* dm_diffmod_create(int device, int cov, double alpha) {
    const char* why = dfk::check_rule(cov, alpha);
    if (why) {
        fail(DM_EINVAL, "dm_diffmod_create: %s (got cov %d alpha %g)", why, cov, alpha);
        return nullptr;
    }
    if (!table_stage_device("dm_diffmod", device)) return nullptr;
    using B = dm_diffmod;
    dm_diffmod* h = new dm_diffmod;
    h->cov = cov;
    h->alpha = alpha;
    const size_t lf_bytes = (size_t(dfk::MAX_TOTAL) + 1) * sizeof(double);
    bool ok = h->open(device, "dm_diffmod");
    ok = ok && h->b.ensure(B::LF, lf_bytes) == DM_OK && h->b.ensure(B::HIST, dfk::HIST_BINS * 8) == DM_OK && h->b.ensure(B::COUNTS, dfk::N_WORDS * 8) == DM_OK;
    ok = ok && hipMemcpyAsync(h->b.buf[B::LF], dfk::lf_table(), lf_bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess;
    ok = ok && h->zero_block(B::HIST, dfk::HIST_BINS * 8) == DM_OK;
    if (!ok) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_diffmod_create: stream, events, table or counters on device %d", device);
        dm_diffmod_destroy(h);
        return nullptr;
    }
    return h;
}

int dm_diffmod_run(dm_diffmod* h, dm_summary* plus, dm_summary* minus, dm_summary* ctrl_plus, dm_summary* ctrl_minus, int64_t* counters, int64_t* n_records) {
    using B = dm_diffmod;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!counters || !n_records) return fail(DM_EINVAL, "dm_diffmod_run: null argument");
    if (!plus || !minus || plus == minus) return fail(DM_EINVAL, "dm_diffmod_run: two sample tables, one per strand (null handle)");
    if (!ctrl_plus || !ctrl_minus) return fail(DM_EINVAL, "dm_diffmod_run: the controls are missing (two tables, one per strand)");
    if (ctrl_plus == ctrl_minus || ctrl_plus == plus || ctrl_plus == minus || ctrl_minus == plus || ctrl_minus == minus)
        return fail(DM_EINVAL, "dm_diffmod_run: the control tables are two tables of their own");
    dm_summary* tab[4] = {plus, minus, ctrl_plus, ctrl_minus};
    const long long len = dm_summary_length(plus);
    if (len < 1 || len > dfk::MAX_LENGTH) return fail(DM_EINVAL, "dm_diffmod_run: tables of %lld positions (1 to 2^31 - 1)", len);
    for (int j = 0; j < 4; ++j)
        if (dm_summary_length(tab[j]) != len)
            return fail(DM_EINVAL, "dm_diffmod_run: tables of different lengths: table %d has %lld positions, table 0 %lld", j, (long long)dm_summary_length(tab[j]), len);
    int rc;
    if ((rc = h->tables_ready("dm_diffmod_run", tab, 4)) != DM_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    h->n_records = 0;
    const long long tiles = (len + dfk::TILE_POS - 1) / dfk::TILE_POS;
    if ((rc = h->b.ensure(B::TILE_N, size_t(tiles) * 4)) != DM_OK || (rc = h->b.ensure(B::TILE_OFF, size_t(tiles) * 8)) != DM_OK) return rc;
    hipStream_t s = h->stream;
    const int* t[4];
    for (int j = 0; j < 4; ++j) t[j] = static_cast<const int*>(dm_summary_device_ptr(tab[j]));
    unsigned long long* d_counts = h->b.ptr<unsigned long long>(B::COUNTS);
    const dim3 grid{unsigned(std::min<long long>(tiles, dfk::MAX_BLOCKS))}, block{dfk::THREADS};
    const dfk::WorkList none = {};
    // 1  the fates: counters, tested keys per tile; their scan
    HIP_TRY(hipMemsetAsync(d_counts, 0, dfk::N_WORDS * 8, s));
    HIP_TRY(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(dfk::select_kernel<false>, grid, block, 0, s, len, t[0], t[1], t[2], t[3], h->cov, h->b.ptr<int>(B::TILE_N), h->b.ptr<const long long>(B::TILE_OFF), none,
                       d_counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dfk::scan_kernel, dim3(1), block, 0, s, h->b.ptr<const int>(B::TILE_N), tiles, h->b.ptr<long long>(B::TILE_OFF), d_counts + dfk::W_WORK);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[1], s));
    long long got[dfk::N_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(got, d_counts, sizeof got, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = add_time(h->ev[0], h->ev[1], h->select_ms)) != DM_OK) return rc;
    for (int j = 0; j < 2 * dfk::N_COUNT; ++j) counters[j] = got[j];
    const long long n_work = got[dfk::W_WORK];
    *n_records = 0;
    if (n_work == 0) return DM_OK;
    // 2  the work list in key order
    for (int which : {int(B::KEY), int(B::CA), int(B::MA), int(B::CB), int(B::MB), int(B::LARGE)})
        if ((rc = h->b.ensure(which, size_t(n_work) * 4)) != DM_OK) return rc;
    if ((rc = h->b.ensure(B::P, size_t(n_work) * 8)) != DM_OK) return rc;
    const long long chunks = (n_work + dfk::CHUNK - 1) / dfk::CHUNK;
    if ((rc = h->b.ensure(B::CHUNK_N, size_t(chunks) * 4)) != DM_OK || (rc = h->b.ensure(B::CHUNK_OFF, size_t(chunks) * 8)) != DM_OK) return rc;
    const dfk::WorkList w = {h->b.ptr<unsigned>(B::KEY), h->b.ptr<int>(B::CA), h->b.ptr<int>(B::MA), h->b.ptr<int>(B::CB), h->b.ptr<int>(B::MB), h->b.ptr<double>(B::P),
                             h->b.ptr<unsigned>(B::LARGE), n_work};
    HIP_TRY(hipEventRecord(h->ev[2], s));
    hipLaunchKernelGGL(dfk::select_kernel<true>, grid, block, 0, s, len, t[0], t[1], t[2], t[3], h->cov, h->b.ptr<int>(B::TILE_N), h->b.ptr<const long long>(B::TILE_OFF), w,
                       d_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], s));
    // 3  the tests: the keys above SMALL_S a workgroup each, then every key a 16-lane group each (which takes the p of a large key as it stands)
    const double* lf = h->b.ptr<const double>(B::LF);
    HIP_TRY(hipEventRecord(h->ev[4], s));
    hipLaunchKernelGGL(dfk::fisher_kernel<true>, dim3(unsigned(std::min<long long>(n_work, dfk::LARGE_BLOCKS))), block, 0, s, lf, w, h->alpha, h->b.ptr<int>(B::CHUNK_N),
                       h->b.ptr<unsigned long long>(B::HIST), d_counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dfk::fisher_kernel<false>, dim3(unsigned(chunks)), block, 0, s, lf, w, h->alpha, h->b.ptr<int>(B::CHUNK_N), h->b.ptr<unsigned long long>(B::HIST),
                       d_counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dfk::scan_kernel, dim3(1), block, 0, s, h->b.ptr<const int>(B::CHUNK_N), chunks, h->b.ptr<long long>(B::CHUNK_OFF), d_counts + dfk::W_RECORDS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[5], s));
    HIP_TRY(hipMemcpyAsync(got, d_counts, sizeof got, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = add_time(h->ev[2], h->ev[3], h->select_ms)) != DM_OK || (rc = add_time(h->ev[4], h->ev[5], h->fisher_ms)) != DM_OK) return rc;
    const long long n_rec = got[dfk::W_RECORDS];
    if (n_rec > 0) {
        // 4  the records in key order
        for (int which : {int(B::R_POS), int(B::R_CA), int(B::R_MA), int(B::R_CB), int(B::R_MB)})
            if ((rc = h->b.ensure(which, size_t(n_rec) * 4)) != DM_OK) return rc;
        if ((rc = h->b.ensure(B::R_STRAND, size_t(n_rec))) != DM_OK || (rc = h->b.ensure(B::R_P, size_t(n_rec) * 8)) != DM_OK) return rc;
        const dfk::Records r = {h->b.ptr<int>(B::R_POS), h->b.ptr<unsigned char>(B::R_STRAND), h->b.ptr<int>(B::R_CA), h->b.ptr<int>(B::R_MA), h->b.ptr<int>(B::R_CB),
                                h->b.ptr<int>(B::R_MB), h->b.ptr<double>(B::R_P), n_rec};
        hipLaunchKernelGGL(dfk::records_kernel, dim3(unsigned(chunks)), block, 0, s, w, h->alpha, h->b.ptr<const long long>(B::CHUNK_OFF), r);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
    }
    h->n_records = n_rec;
    *n_records = n_rec;
    return DM_OK;
}

int dm_diffmod_fetch_records(dm_diffmod* h, int64_t first, int64_t count, int32_t* pos, uint8_t* strand, int32_t* cA, int32_t* mA, int32_t* cB, int32_t* mB, double* p) {
    using B = dm_diffmod;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (first < 0 || count < 0 || first + count > h->n_records)
        return fail(DM_EINVAL, "dm_diffmod_fetch_records: records %lld .. %lld of %lld", (long long)first, (long long)(first + count), h->n_records);
    if (count == 0) return DM_OK;
    if (!pos || !strand || !cA || !mA || !cB || !mB || !p) return fail(DM_EINVAL, "dm_diffmod_fetch_records: null argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t n = size_t(count), f = size_t(first);
    HIP_TRY(hipMemcpyAsync(pos, h->b.ptr<int>(B::R_POS) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(strand, h->b.ptr<unsigned char>(B::R_STRAND) + f, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cA, h->b.ptr<int>(B::R_CA) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(mA, h->b.ptr<int>(B::R_MA) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cB, h->b.ptr<int>(B::R_CB) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(mB, h->b.ptr<int>(B::R_MB) + f, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p, h->b.ptr<double>(B::R_P) + f, n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

int dm_diffmod_fetch_hist(dm_diffmod* h, int64_t* hist) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!hist) return fail(DM_EINVAL, "dm_diffmod_fetch_hist: null argument");
    return h->fetch_block(dm_diffmod::HIST, hist, dfk::HIST_BINS * 8);
}

int dm_diffmod_reset(dm_diffmod* h) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->n_records = 0;
    return h->zero_block(dm_diffmod::HIST, dfk::HIST_BINS * 8);
}

int dm_diffmod_times(dm_diffmod* h, double* select_ms, double* fisher_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (select_ms) *select_ms = h->select_ms;
    if (fisher_ms) *fisher_ms = h->fisher_ms;
    return DM_OK;
}

}  // extern "C"
#endif  // the handle
