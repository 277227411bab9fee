// siteperf.hip.inc — `siteperf`, device part (part of offline.hip): the BED lines of a run and of its control runs ->
// the histograms every site-level curve of DeepMod_tools/cal_EcoliDetPerf.py is a function of.
//   readFA (:31-74)                        sp_code_kernel   one byte per position: bit 0 = '+' site, bit 1 = '-' site, inside start..end only
//   readmodf (:134-176)                    sp_count_kernel  a run line -> its category (:222), label (1 iff a site) and coverage bucket -> one count
//   readmodf_dict (:76-104)                sp_scatter_kernel  a control line -> coverage and modified count summed per (position, strand)
//   add_from_dict (:106-131)               sp_walk_kernel   every (position, strand) a control line named -> one label-0 entry, pct = (100 mod) / cov
// deepmod_amd/siteperf.py (HostEngine) is the numpy twin of these kernels and the statement of the semantics.
//
// The text of a file is split into lines by textlines.hip.inc (xlk::split), then sp_parse_kernel reads one line per lane with spk::parse_line
// (siteperf.inc, where the device grammar is stated).  A line outside it ('\r', an empty line, two separators, another contig, a sign ...) is
// marked: the call reports the first of them and counts nothing, and the caller sends the file through its own parser and
// dm_siteperf_add_records.
//
// Exactness.  Everything counted is an integer: the histogram hist[category 7][label 2][bucket][percentage 101] (bucket = thresholds <=
// coverage, minus one; below the smallest threshold: no count), the read-level sums tp / fp / tn / fn and the line counters.  A block counts
// into a private LDS histogram of 32-bit counters (a block sees fewer than 2^32 records) and adds its non-zero bins to the global 64-bit
// counters once; the sums are reduced per wave and added with one 64-bit atomic per wave.  Integer additions commute and associate, so the
// result does not depend on the order the atomics land in: two runs give the same bytes, and they are the twin's.
// The control tables take int32 atomic adds (the caller's contract: the per-file largest coverages of a contig sum to < 2^31, a site at most
// once per file; the walk refuses a sum that is negative or whose modified count exceeds its coverage).  "The base of the first line seen"
// (:100) needs an order that atomics do not give: every control line carries the key (file index << 40 | line index) << 8 | base, and a
// 64-bit atomic min per (position, strand) keeps the smallest: the first line of the first file, whatever the schedule.
#pragma once
#include "host.h"
#include "xyrows.hip.inc"
#include "textlines.hip.inc"
#include "siteperf.inc"

namespace spk {

constexpr int THREADS = 256;
constexpr int MAX_MOTIF = 16;
constexpr int MAX_THR = 8;
constexpr int NCAT = 7;                             // M, M_n1B, M_n2B, M_n3B, OtherB, M_nb, Other (:222)
constexpr int NPCT = 101;
constexpr int MAX_BLOCKS = 1024;                    // grid of the record kernels: a block loops over its share and flushes once
constexpr unsigned long long NO_KEY = ~0ull;
enum { S_TP, S_FP, S_TN, S_FN, S_SKIPPED, S_MISMATCH, S_MAXCOV, S_BADSUM, N_STAT };

struct Motif {
    unsigned char pat[MAX_MOTIF], rc[MAX_MOTIF];    // the motif in upper case, its reverse complement
    int m, k;
    unsigned char B;                                // motif[k] as typed
};
struct Thr {
    int t[MAX_THR];                                 // ascending
    int n;
};
struct Recs {                                       // one BED line each
    const int *pos, *cov, *pct, *mod;
    const unsigned char *strand, *base;             // strand 0 '+', 1 '-'
};

__host__ __device__ inline unsigned char complement(const unsigned char b) {       // na4com (:29); anything else equals no base
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : 0;
}

__device__ inline bool matches(const unsigned char* __restrict__ seq, const long long len, const long long first, const unsigned char* pat, const int m) {
    if (first < 0 || first + m > len) return false;
    for (int j = 0; j < m; ++j)
        if (seq[first + j] != pat[j]) return false;                  // case-sensitive on the FASTA bytes, as the reference
    return true;
}

__global__ __launch_bounds__(THREADS) void sp_code_kernel(const unsigned char* __restrict__ seq, const long long len, const Motif mo, const long long lo, const long long hi,
                                                         unsigned char* __restrict__ code) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= len) return;
    unsigned char c = 0;
    if (i >= lo && i <= hi) {
        if (matches(seq, len, i - mo.k, mo.pat, mo.m)) c |= 1;
        if (matches(seq, len, i - (mo.m - 1 - mo.k), mo.rc, mo.m)) c |= 2;
    }
    code[i] = c;
}

__global__ __launch_bounds__(THREADS) void sp_parse_kernel(const char* __restrict__ text, const long long* __restrict__ start, const long long n_rows, const bed::Name name,
                                                          const long long contig_len, int* __restrict__ pos, int* __restrict__ cov, int* __restrict__ pct,
                                                          int* __restrict__ mod, unsigned char* __restrict__ strand, unsigned char* __restrict__ base,
                                                          unsigned char* __restrict__ status) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const long long b = start[r], e = start[r + 1] - 1;              // text[e] is the line's '\n'
    Rec v = {0, 0, 0, 0, 0, 0};
    const bool ok = parse_line(text + b, e - b, name, contig_len, v);
    pos[r] = ok ? v.pos : 0;
    cov[r] = ok ? v.cov : 0;
    pct[r] = ok ? v.pct : 0;
    mod[r] = ok ? v.mod : 0;
    strand[r] = ok ? v.strand : 0;
    base[r] = ok ? v.base : 0;
    status[r] = ok ? 0 : 1;
}

// the category of (strand s, position pos, line base equal to B or not); code holds len bytes, 0 <= pos < len
__device__ inline int category(const unsigned char* __restrict__ code, const long long len, const long long pos, const int s, const bool is_b) {
    const unsigned bit = 1u << s;
    if (code[pos] & bit) return 0;
    int near = 0;
    const int offs[6] = {-3, -2, -1, 1, 2, 3};                       // range(-3, 4) of :119: the first offset with a site decides
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const long long q = pos + offs[j];
        if (near == 0 && q >= 0 && q < len && (code[q] & bit)) near = offs[j] < 0 ? -offs[j] : offs[j];
    }
    if (is_b) return near ? near : 4;
    return near ? 5 : 6;
}

__device__ inline int bucket_of(const Thr& thr, const int cov) {
    int b = 0;
#pragma unroll
    for (int j = 0; j < MAX_THR; ++j) b += (j < thr.n && thr.t[j] <= cov) ? 1 : 0;
    return b;
}

// every lane of the wave calls it; one 64-bit atomic per wave with something to add
__device__ inline void wave_add(unsigned long long* dst, long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(dst, (unsigned long long)v);
}

__device__ inline void zero_bins(unsigned* lh, const int bins) {
    for (int j = threadIdx.x; j < bins; j += THREADS) lh[j] = 0;
    __syncthreads();
}

// lh [NCAT][nt][NPCT] of the block -> hist [NCAT][2][nt][NPCT]; label_m: the label of the entries of category 0 (every other entry has label 0)
__device__ inline void flush_bins(const unsigned* lh, const int nt, const int label_m, unsigned long long* __restrict__ hist) {
    __syncthreads();
    const int per_cat = nt * NPCT;
    for (int j = threadIdx.x; j < NCAT * per_cat; j += THREADS) {
        const unsigned v = lh[j];
        if (!v) continue;
        const int cat = j / per_cat, rem = j - cat * per_cat;
        atomicAdd(&hist[(long long)(cat * 2 + (cat == 0 ? label_m : 0)) * per_cat + rem], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(THREADS) void sp_count_kernel(const Recs r, const long long n, const unsigned char* __restrict__ code, const unsigned char* __restrict__ seq,
                                                          const long long len, const long long lo, const long long hi, const unsigned char B, const Thr thr,
                                                          unsigned long long* __restrict__ hist, unsigned long long* __restrict__ stat) {
    __shared__ unsigned lh[NCAT * MAX_THR * NPCT];
    zero_bins(lh, NCAT * thr.n * NPCT);
    long long tp = 0, fp = 0, tn = 0, fn = 0, skipped = 0, mism = 0;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) {
        const long long pos = r.pos[i];
        if (pos < lo || pos > hi) {
            ++skipped;
            continue;
        }
        const int s = r.strand[i] & 1;
        const unsigned char base = r.base[i];
        const unsigned char refb = s ? complement(seq[pos]) : seq[pos];
        if (base != B || base != refb) ++mism;                       // :153
        const int cat = category(code, len, pos, s, base == B);
        const int cv = r.cov[i], md = r.mod[i];
        if (cat == 0) {
            tp += md;
            fn += cv - md;
        } else {
            fp += md;
            tn += cv - md;
        }
        const int b = bucket_of(thr, cv);
        if (b > 0) atomicAdd(&lh[(cat * thr.n + b - 1) * NPCT + r.pct[i]], 1u);
    }
    flush_bins(lh, thr.n, 1, hist);
    wave_add(stat + S_TP, tp);
    wave_add(stat + S_FP, fp);
    wave_add(stat + S_TN, tn);
    wave_add(stat + S_FN, fn);
    wave_add(stat + S_SKIPPED, skipped);
    wave_add(stat + S_MISMATCH, mism);
}

// tab [len][2 strands][cov | mod], key [len][2 strands]
__global__ __launch_bounds__(THREADS) void sp_scatter_kernel(const Recs r, const long long n, const unsigned char* __restrict__ seq, const long long lo, const long long hi,
                                                            const unsigned char B, const unsigned long long file_index, int* __restrict__ tab,
                                                            unsigned long long* __restrict__ key, unsigned long long* __restrict__ stat) {
    long long skipped = 0, mism = 0;
    int cmax = 0;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) {
        const long long pos = r.pos[i];
        if (pos < lo || pos > hi) {
            ++skipped;
            continue;
        }
        const int s = r.strand[i] & 1;
        const unsigned char base = r.base[i];
        const unsigned char refb = s ? complement(seq[pos]) : seq[pos];
        if (base != B || base != refb) ++mism;                       // :96
        const int cv = r.cov[i];
        const long long e = pos * 2 + s;
        atomicAdd(&tab[e * 2], cv);
        atomicAdd(&tab[e * 2 + 1], r.mod[i]);
        atomicMin(&key[e], (((file_index << 40) | (unsigned long long)i) << 8) | base);
        cmax = max(cmax, cv);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cmax = max(cmax, __shfl_down(cmax, d, 64));
    if ((threadIdx.x & 63) == 0 && cmax > 0) atomicMax(stat + S_MAXCOV, (unsigned long long)cmax);
    wave_add(stat + S_SKIPPED, skipped);
    wave_add(stat + S_MISMATCH, mism);
}

__global__ __launch_bounds__(THREADS) void sp_walk_kernel(const int* __restrict__ tab, const unsigned long long* __restrict__ key, const unsigned char* __restrict__ code,
                                                         const long long len, const unsigned char B, const Thr thr, unsigned long long* __restrict__ hist,
                                                         unsigned long long* __restrict__ stat) {
    __shared__ unsigned lh[NCAT * MAX_THR * NPCT];
    zero_bins(lh, NCAT * thr.n * NPCT);
    long long fp = 0, tn = 0, bad = 0;
    for (long long e = (long long)blockIdx.x * THREADS + threadIdx.x; e < 2 * len; e += (long long)gridDim.x * THREADS) {
        const unsigned long long k = key[e];
        if (k == NO_KEY) continue;
        const int cv = tab[e * 2], md = tab[e * 2 + 1];
        if (cv < 0 || md < 0 || md > cv) {
            ++bad;
            continue;
        }
        const int pct = cv > 0 ? int((100ll * md) / cv) : 0;         // int(mod * 100 / cov) of the sums (:104)
        const int cat = category(code, len, e >> 1, int(e & 1), (unsigned char)(k & 0xffull) == B);
        fp += md;
        tn += cv - md;
        const int b = bucket_of(thr, cv);
        if (b > 0) atomicAdd(&lh[(cat * thr.n + b - 1) * NPCT + pct], 1u);
    }
    flush_bins(lh, thr.n, 0, hist);
    wave_add(stat + S_FP, fp);
    wave_add(stat + S_TN, tn);
    wave_add(stat + S_BADSUM, bad);
}

}  // namespace spk

struct dm_siteperf {
    dm_xyrows* xy = nullptr;                            // stream, the scan and its block sums
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    enum { POS = xlk::N_SPLIT, COV, PCT, MOD, STRAND, BASE, SEQ, CODE, TAB, KEY, HIST, STAT, N_BUF };
    DevBufs<N_BUF> b{"dm_siteperf"};
    spk::Thr thr = {};
    spk::Motif motif = {};
    int64_t len = -1, lo = 0, hi = -1;                  // the open contig (len < 0: none) and its region, clipped to the contig
    int64_t n_records = 0;                              // records on the device, of the last add_text / add_records
    int64_t control_files = 0, control_cov = 0;         // of the open contig: control calls so far, the sum of their largest coverages
    int64_t lines_seen = 0;
    double parse_ms = 0.0, count_ms = 0.0;
};

namespace spk {

constexpr int64_t MAX_RECORDS = 0x7fffffffLL;

// motif[0 .. m) (1 <= m <= MAX_MOTIF, 0 <= k < m: the caller's check) in upper case and its reverse complement -> mo; -> -1, or the offset
// the reverse complement meets first of a letter that is none of A, C, G, T.  What sp_code_kernel takes: dm_siteperf_set_contig and dm_bslabels_open (bslabels.hip.inc)
inline int make_motif(Motif& mo, const char* motif, const int m, const int k) {
    mo = {};
    mo.m = m;
    mo.k = k;
    mo.B = (unsigned char)motif[k];
    for (int j = 0; j < m; ++j) {
        const unsigned char c = (unsigned char)motif[j];
        mo.pat[j] = (c >= 'a' && c <= 'z') ? c - 32 : c;
    }
    for (int j = 0; j < m; ++j) {
        mo.rc[j] = complement(mo.pat[m - 1 - j]);
        if (!mo.rc[j]) return m - 1 - j;
    }
    return -1;
}
constexpr int64_t MAX_CONTROL_FILES = int64_t(1) << 16;              // the key holds 16 bits of file index, 40 of line index, 8 of base

int record_buffers(dm_siteperf* h, int64_t n) {
    using B = dm_siteperf;
    int rc;
    for (int which : {int(B::POS), int(B::COV), int(B::PCT), int(B::MOD)})
        if ((rc = h->b.ensure(which, size_t(n) * 4)) != DM_OK) return rc;
    for (int which : {int(B::STRAND), int(B::BASE), int(xlk::STATUS)})
        if ((rc = h->b.ensure(which, size_t(n))) != DM_OK) return rc;
    return DM_OK;
}

// the n records on the device -> the histograms (run) or the control tables
int count_records(dm_siteperf* h, int role, int64_t n) {
    using B = dm_siteperf;
    h->lines_seen += n;
    if (n == 0) return DM_OK;
    hipStream_t s = h->xy->stream;
    const Recs r = {h->b.ptr<const int>(B::POS), h->b.ptr<const int>(B::COV), h->b.ptr<const int>(B::PCT), h->b.ptr<const int>(B::MOD),
                    h->b.ptr<const unsigned char>(B::STRAND), h->b.ptr<const unsigned char>(B::BASE)};
    const dim3 grid{unsigned(std::min<int64_t>((n + THREADS - 1) / THREADS, MAX_BLOCKS))}, block{THREADS};
    unsigned long long* d_stat = h->b.ptr<unsigned long long>(B::STAT);
    if (role == 1) {
        if (h->control_files >= MAX_CONTROL_FILES) return fail(DM_EINVAL, "dm_siteperf: more than %lld control files of one contig", (long long)MAX_CONTROL_FILES);
        HIP_TRY(hipMemsetAsync(d_stat + S_MAXCOV, 0, 8, s));
    }
    HIP_TRY(hipEventRecord(h->ev[2], s));
    if (role == 0)
        hipLaunchKernelGGL(sp_count_kernel, grid, block, 0, s, r, (long long)n, h->b.ptr<const unsigned char>(B::CODE), h->b.ptr<const unsigned char>(B::SEQ), (long long)h->len,
                           (long long)h->lo, (long long)h->hi, h->motif.B, h->thr, h->b.ptr<unsigned long long>(B::HIST), d_stat);
    else
        hipLaunchKernelGGL(sp_scatter_kernel, grid, block, 0, s, r, (long long)n, h->b.ptr<const unsigned char>(B::SEQ), (long long)h->lo, (long long)h->hi, h->motif.B,
                           (unsigned long long)h->control_files, h->b.ptr<int>(B::TAB), h->b.ptr<unsigned long long>(B::KEY), d_stat);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], s));
    unsigned long long maxcov = 0;
    if (role == 1) HIP_TRY(hipMemcpyAsync(&maxcov, d_stat + S_MAXCOV, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int rc = add_time(h->ev[2], h->ev[3], h->count_ms);
    if (rc) return rc;
    if (role == 1) {
        ++h->control_files;
        h->control_cov += int64_t(maxcov);
        if (h->control_cov >= (int64_t(1) << 31))
            return fail(DM_EINVAL, "dm_siteperf: the largest coverages of this contig's control files sum to %lld (2^31 or more): the int32 tables cannot hold them",
                        (long long)h->control_cov);
    }
    return DM_OK;
}

}  // namespace spk

extern "C" {

int dm_siteperf_tile_bytes(void) { return xlk::TILE; }

void dm_siteperf_destroy(dm_siteperf* h) {
    if (!h) return;
    if (h->xy) {
        (void)hipSetDevice(h->xy->device);
        (void)hipStreamSynchronize(h->xy->stream);
    }
    h->b.release();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    dm_xy_destroy(h->xy);
    delete h;
}

dm_siteperf* dm_siteperf_create(int device, int n_thresholds, const int32_t* thresholds) {
    if (n_thresholds < 1 || n_thresholds > spk::MAX_THR || !thresholds) {
        fail(DM_EINVAL, "dm_siteperf_create: %d thresholds (1 to %d)", n_thresholds, spk::MAX_THR);
        return nullptr;
    }
    for (int j = 0; j < n_thresholds; ++j)
        if (thresholds[j] < 0 || (j > 0 && thresholds[j] <= thresholds[j - 1])) {
            fail(DM_EINVAL, "dm_siteperf_create: the thresholds are non-negative and strictly ascending (threshold %d is %d)", j, thresholds[j]);
            return nullptr;
        }
    dm_xyrows* xy = dm_xy_create(device);
    if (!xy) return nullptr;
    dm_siteperf* h = new dm_siteperf;
    h->xy = xy;
    h->thr.n = n_thresholds;
    for (int j = 0; j < n_thresholds; ++j) h->thr.t[j] = thresholds[j];
    bool ok = true;
    for (hipEvent_t& e : h->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    const size_t hist_bytes = size_t(spk::NCAT) * 2 * n_thresholds * spk::NPCT * 8;
    ok = ok && h->b.ensure(dm_siteperf::HIST, hist_bytes) == DM_OK && h->b.ensure(dm_siteperf::STAT, spk::N_STAT * 8) == DM_OK;
    ok = ok && hipMemsetAsync(h->b.buf[dm_siteperf::HIST], 0, hist_bytes, xy->stream) == hipSuccess &&
         hipMemsetAsync(h->b.buf[dm_siteperf::STAT], 0, spk::N_STAT * 8, xy->stream) == hipSuccess && hipStreamSynchronize(xy->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_siteperf_create: events or counters on device %d", device);
        dm_siteperf_destroy(h);
        return nullptr;
    }
    return h;
}

int dm_siteperf_set_contig(dm_siteperf* h, const uint8_t* seq, int64_t len, const char* motif, int m, int k, int64_t start, int64_t end) {
    using B = dm_siteperf;
    if (!h) return fail(DM_EINVAL, "null handle");
    h->len = -1;
    if (len < 1 || len > 0x7fffffffLL || !seq) return fail(DM_EINVAL, "dm_siteperf_set_contig: a contig of %lld bases (1 to 2^31 - 1)", (long long)len);
    if (!motif || m < 1 || m > spk::MAX_MOTIF || k < 0 || k >= m)
        return fail(DM_EINVAL, "dm_siteperf_set_contig: motif of %d bases (1 to %d), modified offset %d", m, spk::MAX_MOTIF, k);
    spk::Motif mo = {};
    const int other = spk::make_motif(mo, motif, m, k);
    if (other >= 0) return fail(DM_EINVAL, "dm_siteperf_set_contig: motif base %d is none of A, C, G, T", other);
    h->motif = mo;
    h->lo = start < 0 ? 0 : start;                                    // a negative bound: none (the reference's -1)
    h->hi = (end < 0 || end > len - 1) ? len - 1 : end;
    HIP_TRY(hipSetDevice(h->xy->device));
    int rc;
    if ((rc = h->b.ensure(B::SEQ, size_t(len))) || (rc = h->b.ensure(B::CODE, size_t(len))) || (rc = h->b.ensure(B::TAB, size_t(len) * 16)) ||
        (rc = h->b.ensure(B::KEY, size_t(len) * 16)))
        return rc;
    hipStream_t s = h->xy->stream;
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::SEQ], seq, size_t(len), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(h->b.buf[B::TAB], 0, size_t(len) * 16, s));
    HIP_TRY(hipMemsetAsync(h->b.buf[B::KEY], 0xff, size_t(len) * 16, s));
    hipLaunchKernelGGL(spk::sp_code_kernel, dim3(unsigned((len + spk::THREADS - 1) / spk::THREADS)), dim3(spk::THREADS), 0, s, h->b.ptr<const unsigned char>(B::SEQ),
                       (long long)len, mo, (long long)h->lo, (long long)h->hi, h->b.ptr<unsigned char>(B::CODE));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    h->len = len;
    h->n_records = 0;
    h->control_files = h->control_cov = 0;
    return DM_OK;
}

int dm_siteperf_fetch_codes(dm_siteperf* h, uint8_t* code) {
    if (!h || !code) return fail(DM_EINVAL, "null argument");
    if (h->len < 0) return fail(DM_ESTATE, "dm_siteperf_fetch_codes: no contig");
    HIP_TRY(hipSetDevice(h->xy->device));
    HIP_TRY(hipMemcpy(code, h->b.buf[dm_siteperf::CODE], size_t(h->len), hipMemcpyDeviceToHost));
    return DM_OK;
}

int64_t dm_siteperf_parse_host(const char* text, int64_t n_bytes, const char* contig_name, int64_t contig_len, int32_t* pos, uint8_t* strand, uint8_t* base, int32_t* cov,
                               int32_t* pct, int32_t* mod, int64_t cap, int32_t* flag, int64_t* first_bad_line) {
    if (n_bytes < 0 || (n_bytes > 0 && !text) || !contig_name || cap < 0 || (cap > 0 && (!pos || !strand || !base || !cov || !pct || !mod)))
        return fail(DM_EINVAL, "dm_siteperf_parse_host: null argument");
    bed::Name name = {};
    if (!bed::set_name(name, contig_name)) return fail(DM_EINVAL, "dm_siteperf_parse_host: a contig name of %zu bytes (1 to %d)", std::strlen(contig_name), bed::MAX_NAME);
    int64_t bad = 0;
    const int64_t rows = spk::parse_text(text, n_bytes, name, contig_len, pos, strand, base, cov, pct, mod, cap, &bad);
    if (flag) *flag = bad != 0;
    if (first_bad_line) *first_bad_line = bad ? bad : -1;
    return rows;
}

int dm_siteperf_add_text(dm_siteperf* h, const char* text, int64_t n_bytes, int role, const char* contig_name, int64_t* n_lines, int32_t* flag, int64_t* first_bad_line) {
    using B = dm_siteperf;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (n_lines) *n_lines = 0;
    if (flag) *flag = 0;
    if (first_bad_line) *first_bad_line = -1;
    if (h->len < 0) return fail(DM_ESTATE, "dm_siteperf_add_text: no contig");
    if (role != 0 && role != 1) return fail(DM_EINVAL, "dm_siteperf_add_text: role %d (0 run, 1 control)", role);
    bed::Name name = {};
    if (!bed::set_name(name, contig_name))
        return fail(DM_EINVAL, "dm_siteperf_add_text: a contig name of %zu bytes (1 to %d)", contig_name ? std::strlen(contig_name) : size_t(0), bed::MAX_NAME);
    h->n_records = 0;
    HIP_TRY(hipSetDevice(h->xy->device));
    int rc;
    long long rows = 0;
    if ((rc = xlk::split(h->xy, h->b, text, n_bytes, spk::MAX_RECORDS, "dm_siteperf_add_text", "lines", h->ev[0], &rows)) != DM_OK || rows == 0) return rc;
    if ((rc = spk::record_buffers(h, rows)) != DM_OK) return rc;
    hipStream_t s = h->xy->stream;
    hipLaunchKernelGGL(spk::sp_parse_kernel, dim3(unsigned((rows + spk::THREADS - 1) / spk::THREADS)), dim3(spk::THREADS), 0, s, h->b.ptr<const char>(xlk::TEXT),
                       h->b.ptr<const long long>(xlk::START), rows, name, (long long)h->len, h->b.ptr<int>(B::POS), h->b.ptr<int>(B::COV), h->b.ptr<int>(B::PCT),
                       h->b.ptr<int>(B::MOD), h->b.ptr<unsigned char>(B::STRAND), h->b.ptr<unsigned char>(B::BASE), h->b.ptr<unsigned char>(xlk::STATUS));
    HIP_TRY(hipGetLastError());
    if ((rc = xlk::first_bad(h->xy, h->b, rows)) != DM_OK) return rc;
    HIP_TRY(hipEventRecord(h->ev[1], s));
    long long first = -1;
    HIP_TRY(hipMemcpyAsync(&first, h->b.buf[xlk::OUT], 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = add_time(h->ev[0], h->ev[1], h->parse_ms)) != DM_OK) return rc;
    if (n_lines) *n_lines = rows;
    if (first >= 0) {                                                // outside the grammar: nothing of this text is counted
        if (flag) *flag = 1;
        if (first_bad_line) *first_bad_line = first + 1;
        return DM_OK;
    }
    h->n_records = rows;
    return spk::count_records(h, role, rows);
}

int dm_siteperf_add_records(dm_siteperf* h, int role, int64_t n, const int32_t* pos, const uint8_t* strand, const uint8_t* base, const int32_t* cov, const int32_t* pct,
                            const int32_t* mod) {
    using B = dm_siteperf;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (h->len < 0) return fail(DM_ESTATE, "dm_siteperf_add_records: no contig");
    if (role != 0 && role != 1) return fail(DM_EINVAL, "dm_siteperf_add_records: role %d (0 run, 1 control)", role);
    if (n < 0 || n > spk::MAX_RECORDS || (n > 0 && (!pos || !strand || !base || !cov || !pct || !mod))) return fail(DM_EINVAL, "dm_siteperf_add_records: %lld records", (long long)n);
    for (int64_t i = 0; i < n; ++i)                                  // what the kernels index with, checked before any launch
        if (pos[i] < 0 || pos[i] >= h->len || strand[i] > 1 || cov[i] < 0 || mod[i] < 0 || mod[i] > cov[i] || pct[i] < 0 || pct[i] > 100)
            return fail(DM_EINVAL, "dm_siteperf_add_records: record %lld (position %d of %lld, strand %d, coverage %d, percentage %d, modified %d)", (long long)i, pos[i],
                        (long long)h->len, int(strand[i]), cov[i], pct[i], mod[i]);
    h->n_records = 0;
    if (n == 0) return DM_OK;
    HIP_TRY(hipSetDevice(h->xy->device));
    int rc = spk::record_buffers(h, n);
    if (rc) return rc;
    hipStream_t s = h->xy->stream;
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::POS], pos, size_t(n) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::COV], cov, size_t(n) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::PCT], pct, size_t(n) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::MOD], mod, size_t(n) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::STRAND], strand, size_t(n), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::BASE], base, size_t(n), hipMemcpyHostToDevice, s));
    h->n_records = n;
    return spk::count_records(h, role, n);
}

int dm_siteperf_fetch_records(dm_siteperf* h, int32_t* pos, uint8_t* strand, uint8_t* base, int32_t* cov, int32_t* pct, int32_t* mod) {
    using B = dm_siteperf;
    if (!h) return fail(DM_EINVAL, "null handle");
    const size_t n = size_t(h->n_records);
    if (n == 0) return DM_OK;
    HIP_TRY(hipSetDevice(h->xy->device));
    if (pos) HIP_TRY(hipMemcpy(pos, h->b.buf[B::POS], n * 4, hipMemcpyDeviceToHost));
    if (cov) HIP_TRY(hipMemcpy(cov, h->b.buf[B::COV], n * 4, hipMemcpyDeviceToHost));
    if (pct) HIP_TRY(hipMemcpy(pct, h->b.buf[B::PCT], n * 4, hipMemcpyDeviceToHost));
    if (mod) HIP_TRY(hipMemcpy(mod, h->b.buf[B::MOD], n * 4, hipMemcpyDeviceToHost));
    if (strand) HIP_TRY(hipMemcpy(strand, h->b.buf[B::STRAND], n, hipMemcpyDeviceToHost));
    if (base) HIP_TRY(hipMemcpy(base, h->b.buf[B::BASE], n, hipMemcpyDeviceToHost));
    return DM_OK;
}

int dm_siteperf_finish_contig(dm_siteperf* h) {
    using B = dm_siteperf;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (h->len < 0) return fail(DM_ESTATE, "dm_siteperf_finish_contig: no contig");
    const int64_t len = h->len;
    h->len = -1;
    h->n_records = 0;
    if (h->control_files == 0) return DM_OK;                         // no control line: no entry
    HIP_TRY(hipSetDevice(h->xy->device));
    hipStream_t s = h->xy->stream;
    unsigned long long* d_stat = h->b.ptr<unsigned long long>(B::STAT);
    const dim3 grid{unsigned(std::min<int64_t>((2 * len + spk::THREADS - 1) / spk::THREADS, spk::MAX_BLOCKS))};
    HIP_TRY(hipEventRecord(h->ev[2], s));
    hipLaunchKernelGGL(spk::sp_walk_kernel, grid, dim3(spk::THREADS), 0, s, h->b.ptr<const int>(B::TAB), h->b.ptr<const unsigned long long>(B::KEY),
                       h->b.ptr<const unsigned char>(B::CODE), (long long)len, h->motif.B, h->thr, h->b.ptr<unsigned long long>(B::HIST), d_stat);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], s));
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_stat + spk::S_BADSUM, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int rc = add_time(h->ev[2], h->ev[3], h->count_ms);
    if (rc) return rc;
    if (bad) return fail(DM_EINVAL, "dm_siteperf_finish_contig: %llu control sums left the int32 range", bad);
    return DM_OK;
}

int dm_siteperf_fetch(dm_siteperf* h, int64_t* hist, int64_t* counts, int64_t* lines_seen, int64_t* lines_skipped, int64_t* base_mismatch) {
    using B = dm_siteperf;
    if (!h) return fail(DM_EINVAL, "null handle");
    HIP_TRY(hipSetDevice(h->xy->device));
    HIP_TRY(hipStreamSynchronize(h->xy->stream));
    long long stat[spk::N_STAT];
    HIP_TRY(hipMemcpy(stat, h->b.buf[B::STAT], sizeof stat, hipMemcpyDeviceToHost));
    if (hist) HIP_TRY(hipMemcpy(hist, h->b.buf[B::HIST], size_t(spk::NCAT) * 2 * h->thr.n * spk::NPCT * 8, hipMemcpyDeviceToHost));
    if (counts)
        for (int j = 0; j < 4; ++j) counts[j] = stat[spk::S_TP + j];
    if (lines_seen) *lines_seen = h->lines_seen;
    if (lines_skipped) *lines_skipped = stat[spk::S_SKIPPED];
    if (base_mismatch) *base_mismatch = stat[spk::S_MISMATCH];
    return DM_OK;
}

int dm_siteperf_times(dm_siteperf* h, double* parse_ms, double* count_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (parse_ms) *parse_ms = h->parse_ms;
    if (count_ms) *count_ms = h->count_ms;
    return DM_OK;
}

}  // extern "C"
