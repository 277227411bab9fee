// signal.hip.inc — raw-signal normalisation and per-event statistics on the GPU (part of feed.hip).
//
// Reference: bin/DeepMod_scripts/myDetect.py
//   :266-282  mnormalized(): over the event-covered slice raw[start_0 : start_last + length_last]
//                 mshift = median(slice)            mscale = median(|slice - mshift|)
//                 raw    = (raw - mshift) / mscale                                  (float64)
//                 med    = median(slice')           mad    = median(|slice' - med|)
//                 raw    = round(clip(raw, med - 5 mad, med + 5 mad), 3)
//   :332-343  per event i: mean_i = round(np.mean(raw[start_i : start_i + length_i]), 3), stdv_i likewise with np.std,
//             stored into '<f4' fields; the loop stops at the first event whose slice is empty.
//
// MI355X mapping.  The raw signal is int16, so every quantity above is a function of the 65,536-bin histogram of the
// slice: the four medians are order statistics of f(x) over the distinct sample values x, and the normalised, clipped,
// rounded signal is a 65,536-entry float64 table.  Per read:
//   1. signal_hist_kernel   HBM-bound, 2 B/sample: 16-byte loads, LDS-privatised histogram (4 copies x 8,192 bins for the
//                           values [-2048, 6144), global atomics for the rest), flushed with one atomic per non-empty bin;
//   2. order statistics     exact, in float64 (numpy's median semantics: mean of the two middle values for even counts)
//                           -> mshift, mscale, med, mad, limits.  Batched call: signal_norm_batch_kernel, one workgroup per read
//                           (compaction of the non-empty bins into LDS, bitonic sorts by the |x - m| keys); single-read call
//                           and the rare reads the kernel hands back (> 4,096 distinct values, zero scale): on the host;
//   3. signal_lut_kernel    table[x] = rint(clip((x - mshift) / mscale) * 1000) / 1000   (IEEE float64, no contraction);
//   4. event_stats_kernel   one thread per event, 2 B/sample + 16 B/event in, 8 B/event out: mean and population std of
//                           table[raw[i]] in numpy's exact summation order (add.reduce: 8,192-element buffers summed
//                           left to right, each with the 8-lane / 128-block pairwise scheme), so results are bit-identical
//                           to the reference's np.mean / np.std, then rint(v * 1000) / 1000 and the cast to float32.
// Nothing here is GEMM-shaped; the kernels are byte/integer work bounded by HBM and the LDS atomic rate.
//
// This file is the HIP half of the stage: the kernels, the handle (its device blocks are one DevBufs) and the calls, a batched call as a sequence of
// named stages (signal_batch_impl).  What a call works out on the host before it touches the device - the checks, the covered slice, the first empty
// event, the BatchPlan whose tables the upload stage copies as they are - is signalplan.inc, plain C++ that the host tests compile without HIP.
#pragma once
#include "host.h"
#include "signalplan.inc"

namespace sig {

constexpr int LDS_BINS = 8192;       // per copy
constexpr int LDS_COPIES = 4;        // lanes l, l+4, ... share a copy: 4x fewer same-address LDS atomics on clustered values
constexpr int LDS_BIN0 = -2048;      // LDS bins cover values [LDS_BIN0, LDS_BIN0 + LDS_BINS); the rest goes to global atomics
constexpr int NP_BUFSIZE = 8192;     // numpy's reduction buffer (elements)
constexpr int PW_BLOCK = 128;        // numpy's pairwise-sum leaf size

__device__ __forceinline__ void hist_body(const short* __restrict__ raw, const long long lo, const long long hi,
                                          unsigned* __restrict__ hist /*[65536], index = value + 32768*/, unsigned* lh,
                                          int* __restrict__ vrange /*optional: smallest sample value of the slice at [0], largest at [vstride] (atomicMin / atomicMax)*/,
                                          const int vstride = 1) {
    {   // 16-byte stores: zeroing the 128 KB of privatised bins is a fixed cost per workgroup
        uint4* z = reinterpret_cast<uint4*>(lh);
        for (int i = threadIdx.x; i < LDS_COPIES * LDS_BINS / 4; i += blockDim.x) z[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    unsigned* mine = lh + (threadIdx.x & (LDS_COPIES - 1)) * LDS_BINS;
    int vmin = 32767, vmax = -32768;
    auto count = [&](const int v) {
        const int b = v - LDS_BIN0;
        vmin = v < vmin ? v : vmin;
        vmax = v > vmax ? v : vmax;
        if (b >= 0 && b < LDS_BINS) atomicAdd(&mine[b], 1u);
        else atomicAdd(&hist[v + 32768], 1u);
    };
    // body: 16-byte aligned groups of 8 samples; head and tail sample by sample
    const long long a0 = (lo + 7) & ~7ll;                  // first 8-sample boundary (raw itself is >= 16-byte aligned)
    const long long a1 = hi & ~7ll;
    const long long gtid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long gstride = (long long)gridDim.x * blockDim.x;
    if (a0 < a1) {
        const int4* v8 = reinterpret_cast<const int4*>(raw);
        for (long long g = a0 / 8 + gtid; g < a1 / 8; g += gstride) {
            const int4 q = v8[g];
            const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                count((int)(short)(w[k] & 0xffff));
                count(w[k] >> 16);
            }
        }
        for (long long i = lo + gtid; i < a0; i += gstride) count(raw[i]);
        for (long long i = a1 + gtid; i < hi; i += gstride) count(raw[i]);
    } else {
        for (long long i = lo + gtid; i < hi; i += gstride) count(raw[i]);
    }
    __syncthreads();
    if (vrange) {
        for (int o = 32; o > 0; o >>= 1) {
            const int a = __shfl_xor(vmin, o, 64), b = __shfl_xor(vmax, o, 64);
            vmin = a < vmin ? a : vmin;
            vmax = b > vmax ? b : vmax;
        }
        if ((threadIdx.x & 63) == 0 && vmin <= vmax) {
            atomicMin(&vrange[0], vmin);
            atomicMax(&vrange[vstride], vmax);
        }
    }
    for (int i = threadIdx.x; i < LDS_BINS; i += blockDim.x) {
        unsigned c = 0;
#pragma unroll
        for (int k = 0; k < LDS_COPIES; ++k) c += lh[k * LDS_BINS + i];
        if (c) atomicAdd(&hist[i + LDS_BIN0 + 32768], c);
    }
}

__global__ void signal_hist_kernel(const short* __restrict__ raw, const long long lo, const long long hi,
                                   unsigned* __restrict__ hist /*[65536], index = value + 32768*/) {
    extern __shared__ __attribute__((aligned(16))) unsigned lh[];     // [LDS_COPIES][LDS_BINS]
    hist_body(raw, lo, hi, hist, lh, nullptr);
}

// many reads per launch: blockIdx.y = read, raw = the reads' samples back to back, [lo, hi) absolute sample indices
// vrange [2][reads]: the smallest | largest sample value of every read's slice (initialised to large / small by the caller's two memsets): the order statistics
// touch the few thousand bins a read really has, not all 65,536 (round 6), and so does the value table of a read whose events all lie inside its slice
__global__ void signal_hist_batch_kernel(const short* __restrict__ raw, const long long* __restrict__ lo, const long long* __restrict__ hi,
                                         unsigned* __restrict__ hist /*[reads][65536]*/, int* __restrict__ vrange) {
    extern __shared__ __attribute__((aligned(16))) unsigned lh[];
    const int r = blockIdx.y;
    hist_body(raw, lo[r], hi[r], hist + size_t(r) * 65536, lh, vrange + r, int(gridDim.y));
}

struct Norm {
    double mshift, mscale, med, mad, lower, upper;
};

__global__ void signal_lut_kernel(double* __restrict__ lut, const Norm p) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // value = i - 32768
    double v = ((double)(i - 32768) - p.mshift) / p.mscale;
    v = v > p.upper ? p.upper : (v < p.lower ? p.lower : v);
    lut[i] = rint(v * 1000.0) / 1000.0;
}

// full[r] = 0: the entries of the values in vrange only - every sample an event of read r touches lies in its covered slice.  full[r] = 1: all 65,536 -
// an event reaches outside the slice (before start_0, e.g. into the open-pore current ahead of the strand, or past start_last + length_last) and may
// touch any value; the reference normalises the whole signal (myDetect.py:275, :282).  The table buffer is reused across calls: an entry left out here
// holds an earlier read's normalisation.
__global__ void signal_lut_batch_kernel(double* __restrict__ lut /*[reads][65536]*/, const Norm* __restrict__ norms, const int* __restrict__ vrange,
                                        const int* __restrict__ full) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (!full[blockIdx.y] && (i - 32768 < vrange[blockIdx.y] || i - 32768 > vrange[gridDim.y + blockIdx.y])) return;      // no event of this read reads the entry
    const Norm p = norms[blockIdx.y];
    double v = ((double)(i - 32768) - p.mshift) / p.mscale;
    v = v > p.upper ? p.upper : (v < p.lower ? p.lower : v);
    lut[size_t(blockIdx.y) * 65536 + i] = rint(v * 1000.0) / 1000.0;
}

// full[r] = 1 for a read with an event whose samples - clamped at the read's end as event_stats_one clamps them - reach outside its covered slice
// [lo, hi) (absolute sample indices).  Only the events a statistics kernel reads count: e - ev_off[r] < n_stat[r] (all of them in the batched call,
// those before first_empty in the resident form).  The caller zeroes full.
__global__ void event_reach_batch_kernel(const unsigned long long* __restrict__ ev_start, const unsigned long long* __restrict__ ev_length,
                                         const long long* __restrict__ ev_off, const long long* __restrict__ n_stat, const long long* __restrict__ lo,
                                         const long long* __restrict__ hi, const long long* __restrict__ raw_off, const int n_reads, const long long n_events,
                                         int* __restrict__ full) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n_events) return;
    int a = 0, b = n_reads - 1;                      // the last read whose first event is <= e
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (ev_off[mid] <= e) a = mid;
        else b = mid - 1;
    }
    const int r = a;
    if (e - ev_off[r] >= n_stat[r]) return;
    const unsigned long long base = (unsigned long long)raw_off[r], n = (unsigned long long)(raw_off[r + 1] - raw_off[r]);
    const unsigned long long st = ev_start[e];
    unsigned long long t = st + ev_length[e];
    if (t > n) t = n;
    if (st < t && (base + st < (unsigned long long)lo[r] || base + t > (unsigned long long)hi[r])) full[r] = 1;
}

__global__ void signal_gather_kernel(const short* __restrict__ raw, const long long n, const double* __restrict__ lut,
                                     double* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride) out[i] = lut[(int)raw[i] + 32768];
}

// numpy pairwise sum of a virtual array a(i), i in [off, off + n), n <= PW_BLOCK
template <class F>
__device__ __forceinline__ double pw_leaf(const F& a, const long long off, const int n) {
#pragma clang fp contract(off)
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r = r + a(off + i);
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a(off + j);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a(off + i + j);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + a(off + i);
    return res;
}

// n <= NP_BUFSIZE: recursive halving (n2 = n / 2 rounded down to a multiple of 8) down to leaves of <= 128
template <class F>
__device__ double pw_buffer(const F& a, const long long off, const int n) {
#pragma clang fp contract(off)
    if (n <= PW_BLOCK) return pw_leaf(a, off, n);
    struct Frame {
        long long off;
        int n, state;
        double left;
    } st[10];
    int sp = 0;
    st[0] = {off, n, 0, 0.0};
    double ret = 0.0;
    while (sp >= 0) {
        Frame& f = st[sp];
        if (f.n <= PW_BLOCK) {
            ret = pw_leaf(a, f.off, f.n);
            --sp;
            continue;
        }
        int n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) {
            f.state = 1;
            st[sp + 1] = {f.off, n2, 0, 0.0};
            ++sp;
        } else if (f.state == 1) {
            f.left = ret;
            f.state = 2;
            st[sp + 1] = {f.off + n2, f.n - n2, 0, 0.0};
            ++sp;
        } else {
            ret = f.left + ret;
            --sp;
        }
    }
    return ret;
}

// np.add.reduce over a contiguous float64 array: buffers of 8,192 elements accumulated left to right from 0.0
template <class F>
__device__ double np_sum(const F& a, const long long n) {
#pragma clang fp contract(off)
    double out = 0.0;
    for (long long s = 0; s < n; s += NP_BUFSIZE) {
        const int m = (int)((n - s) < NP_BUFSIZE ? (n - s) : NP_BUFSIZE);
        out = out + pw_buffer(a, s, m);
    }
    return out;
}

// one event: mean and population std of lut[raw[s .. min(s + len, n_raw))] in numpy's summation order
__device__ __forceinline__ void event_stats_one(const short* __restrict__ raw, const long long n_raw, const double* __restrict__ lut,
                                                const unsigned long long s, const unsigned long long len, float* mean_out, float* stdv_out) {
#pragma clang fp contract(off)
    unsigned long long t = s + len;
    if (t > (unsigned long long)n_raw) t = (unsigned long long)n_raw;      // numpy slices clamp at the end
    if (s >= t) {                                                          // empty slice: the reference stops here
        *mean_out = __builtin_nanf("");
        *stdv_out = __builtin_nanf("");
        return;
    }
    const long long n = (long long)(t - s);
    const short* seg = raw + s;
    auto val = [&](const long long i) { return lut[(int)seg[i] + 32768]; };
    const double mean = np_sum(val, n) / (double)n;
    auto dev2 = [&](const long long i) {
        const double d = lut[(int)seg[i] + 32768] - mean;
        return d * d;
    };
    const double sd = sqrt(np_sum(dev2, n) / (double)n);
    *mean_out = (float)(rint(mean * 1000.0) / 1000.0);
    *stdv_out = (float)(rint(sd * 1000.0) / 1000.0);
}

__global__ void event_stats_kernel(const short* __restrict__ raw, const long long n_raw, const double* __restrict__ lut,
                                   const unsigned long long* __restrict__ ev_start,
                                   const unsigned long long* __restrict__ ev_length, const long long n_events,
                                   float* __restrict__ ev_mean, float* __restrict__ ev_stdv) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n_events) return;
    event_stats_one(raw, n_raw, lut, ev_start[e], ev_length[e], ev_mean + e, ev_stdv + e);
}

// all events of many reads in one launch: ev_read[e] = the read of event e, starts relative to the read's first sample
__global__ void event_stats_batch_kernel(const short* __restrict__ raw, const long long* __restrict__ raw_off, const double* __restrict__ lut,
                                         const unsigned long long* __restrict__ ev_start, const unsigned long long* __restrict__ ev_length,
                                         const int* __restrict__ ev_read, const long long n_events, float* __restrict__ ev_mean,
                                         float* __restrict__ ev_stdv) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n_events) return;
    const int r = ev_read[e];
    const long long base = raw_off[r];
    event_stats_one(raw + base, raw_off[r + 1] - base, lut + size_t(r) * 65536, ev_start[e], ev_length[e], ev_mean + e, ev_stdv + e);
}

// The RESIDENT form (round 6, dm_signal_event_stats_device): the statistics do not go back to the host.  ev3[e] = (mean, stdv, length) of merged event e
// of the batch - exactly the three values get_Feature (myDetect.py:892-900) puts into a feature row - written where rows_assemble_kernel reads them.
// An event at or behind its read's first empty event keeps the basecaller's values (fb_mean / fb_stdv: the reference's loop stops there, :334-340);
// the read of an event is found by binary search over the event offsets (a wave's 64 events nearly always share it).  flag bit 0: a mean or stdv
// this kernel computed (an event before its read's first empty one) that the split-f16 classifier kernels refuse (|v| > 65504 or NaN) - the batch then
// runs the fp32 kernel.  Lengths and fall-back values are host data: dm_rows_emit_resident range-checks those of the events rows show, and an event no
// row shows does not decide the kernel (as in the host-statistics form, which checks the rows only).
__global__ void event_ev3_batch_kernel(const short* __restrict__ raw, const long long* __restrict__ raw_off, const double* __restrict__ lut,
                                       const unsigned long long* __restrict__ ev_start, const unsigned long long* __restrict__ ev_length,
                                       const long long* __restrict__ ev_off, const long long* __restrict__ n_stat, const int n_reads, const long long n_events,
                                       const float* __restrict__ fb_mean, const float* __restrict__ fb_stdv, float* __restrict__ ev3, int* __restrict__ flag) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n_events) return;
    int lo = 0, hi = n_reads - 1;                    // the last read whose first event is <= e
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ev_off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    const int r = lo;
    const unsigned long long len = ev_length[e];
    float mean, stdv;
    if (e - ev_off[r] < n_stat[r]) {
        const long long base = raw_off[r];
        event_stats_one(raw + base, raw_off[r + 1] - base, lut + size_t(r) * 65536, ev_start[e], len, &mean, &stdv);
        if (!(fabsf(mean) <= 65504.0f) || !(fabsf(stdv) <= 65504.0f)) atomicOr(flag, 1);
    } else {
        mean = fb_mean ? fb_mean[e] : __builtin_nanf("");
        stdv = fb_stdv ? fb_stdv[e] : __builtin_nanf("");
    }
    ev3[3 * e] = mean;
    ev3[3 * e + 1] = stdv;
    ev3[3 * e + 2] = (float)(double)len;
}

// ---- event tables from basecaller move tables (detect --move; dm_signal_move_stats_device) ----
// Reference: MoveTable.py:7-54.  A boundary is a table index i in 1 .. L-1 with move[i] == 1; boundary number k (0-based, in table order) starts event
// k + 1 at first + 2 i, event 0 starts at first, the last event ends at the read's last sample.  That is a segmented count-and-compact over one byte per
// two samples.  The tables of the batch lie back to back; read r's table is cut into chunks of MOVE_CHUNK bytes counted from its 16-byte-aligned base
// (mv_off[r] & ~15), so that every lane loads one aligned 16-byte word; chunk_off[r] = first chunk of read r (host arithmetic over <= 4,096 reads).
//   1. move_count_kernel   one workgroup per chunk: the number of boundaries in it and the table index of its last one;
//   2. move_scan_kernel    one workgroup per read: exclusive scan of its chunks' counts, then the read's status (dm_move_events' rules: the count
//                          against the expected event count, the last boundary and `first` against the read's samples), n_stat and start[0];
//                          an invalid read's slots are zeroed here and nothing else ever writes them;
//   3. move_write_kernel   one workgroup per chunk again: rank of a boundary = chunk base + lanes before it (five __ballot / __popcll rounds over the
//                          bits of the lanes' counts) + earlier bits of its own lane's word -> start[rank + 1];
//   4. move_length_kernel  one thread per event: length[k] = start[k + 1] - start[k], the last one from the read's sample count.
// No atomics: every output has exactly one writer, so the tables are the same bits whatever the scheduling.  Every store is guarded by the read's
// status and its expected event count.
constexpr int MOVE_THREADS = 256;
static_assert(MOVE_CHUNK == MOVE_THREADS * 16, "a workgroup takes one 16-byte word per lane: the table bytes the plan counts chunks in (signalplan.inc)");

// the last read whose first chunk / event is <= c (reads without chunks / events share an offset with their successor and are never chosen)
__device__ __forceinline__ int move_find_read(const long long* __restrict__ off, const int n_reads, const long long c) {
    int a = 0, b = n_reads - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (off[mid] <= c) a = mid;
        else b = mid - 1;
    }
    return a;
}

// bit j set: byte j of the lane's 16-byte word (absolute table byte a + j) is a boundary of the read whose table is [t0, t1): equal to 1, behind the
// read's index 0 and before its end.  Bytes of a neighbouring read (or behind the last table) that the aligned word holds are masked off.
__device__ __forceinline__ unsigned move_mask16(const unsigned char* __restrict__ move, const long long a, const long long t0, const long long t1) {
    if (a >= t1 || a + 16 <= t0 + 1) return 0u;
    const uint4 q = *reinterpret_cast<const uint4*>(move + a);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int b = 0; b < 4; ++b) m |= (((w[k] >> (8 * b)) & 0xffu) == 1u ? 1u : 0u) << (4 * k + b);
    const long long jlo = t0 + 1 - a, jhi = t1 - a;                 // valid bytes: jlo <= j < jhi
    const unsigned lo = jlo <= 0 ? 0u : (1u << (unsigned)jlo) - 1u;  // (jlo <= 15 here)
    const unsigned hi = jhi >= 16 ? 0xffffu : (1u << (unsigned)jhi) - 1u;
    return m & hi & ~lo;
}

// number of boundaries in the lanes before this one (wave64): the lanes' counts are <= 16, so five ballots - one per bit of the count - and the
// population count of each ballot below the lane.  *total = the wave's count.
__device__ __forceinline__ int move_wave_prefix(const int cnt, int* total) {
    const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
    int pre = 0, tot = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        const unsigned long long v = __ballot((cnt >> b) & 1);
        pre += __popcll(v & below) << b;
        tot += __popcll(v) << b;
    }
    *total = tot;
    return pre;
}

__global__ __launch_bounds__(MOVE_THREADS) void move_count_kernel(const unsigned char* __restrict__ move, const long long* __restrict__ mv_off,
                                                                  const long long* __restrict__ chunk_off, const int n_reads,
                                                                  int* __restrict__ ccnt, int* __restrict__ clast) {
    __shared__ int w_cnt[MOVE_THREADS / 64], w_last[MOVE_THREADS / 64];
    const long long c = blockIdx.x;
    const int r = move_find_read(chunk_off, n_reads, c);
    const long long t0 = mv_off[r], t1 = mv_off[r + 1];
    const long long a = (t0 & ~15ll) + (c - chunk_off[r]) * MOVE_CHUNK + threadIdx.x * 16;
    const unsigned m = move_mask16(move, a, t0, t1);
    int tot;
    (void)move_wave_prefix(__popc(m), &tot);
    // the wave's last boundary: the highest bit of the highest lane that has one (table index relative to the read; -1: none)
    const unsigned long long has = __ballot(m != 0u);
    const int mine = m ? int(a - t0) + 31 - __clz(m) : -1;
    const int last = has ? __shfl(mine, 63 - __clzll(has), 64) : -1;
    if ((threadIdx.x & 63) == 0) {
        w_cnt[threadIdx.x >> 6] = tot;
        w_last[threadIdx.x >> 6] = last;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0, l = -1;
#pragma unroll
        for (int k = 0; k < MOVE_THREADS / 64; ++k) {
            n += w_cnt[k];
            l = w_last[k] > l ? w_last[k] : l;
        }
        ccnt[c] = n;
        clast[c] = l;
    }
}

__global__ __launch_bounds__(MOVE_THREADS) void move_scan_kernel(const int* __restrict__ ccnt, const int* __restrict__ clast, const long long* __restrict__ chunk_off,
                                                                 const long long* __restrict__ first, const long long* __restrict__ raw_off,
                                                                 const long long* __restrict__ ev_off, int* __restrict__ cbase, int* __restrict__ status,
                                                                 long long* __restrict__ n_stat, unsigned long long* __restrict__ ev_start,
                                                                 unsigned long long* __restrict__ ev_length) {
    __shared__ int sh[MOVE_THREADS];
    __shared__ int sh_status;
    const int r = blockIdx.x, tid = threadIdx.x;
    const long long c0 = chunk_off[r], nch = chunk_off[r + 1] - c0;
    long long carry = 0;            // boundaries of the chunks before this tile (the same value in every thread)
    int last = -1;
    for (long long t = 0; t < nch; t += MOVE_THREADS) {
        const long long i = t + tid;
        const int v = i < nch ? ccnt[c0 + i] : 0;
        if (i < nch) last = clast[c0 + i] > last ? clast[c0 + i] : last;
        sh[tid] = v;
        __syncthreads();
        for (int o = 1; o < MOVE_THREADS; o <<= 1) {
            const int x = tid >= o ? sh[tid - o] : 0;
            __syncthreads();
            sh[tid] += x;
            __syncthreads();
        }
        if (i < nch) cbase[c0 + i] = int(carry) + sh[tid] - v;
        carry += sh[MOVE_THREADS - 1];
        __syncthreads();
    }
    sh[tid] = last;
    __syncthreads();
    for (int o = MOVE_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] = sh[tid + o] > sh[tid] ? sh[tid + o] : sh[tid];
        __syncthreads();
    }
    const long long e0 = ev_off[r], nrow = ev_off[r + 1] - e0, nsig = raw_off[r + 1] - raw_off[r], f = first[r];
    if (tid == 0) {
        int st = 0;
        if (carry != nrow - 1) st = 1;                                                       // DM_MOVE_COUNT
        else if (f < 0 || f >= nsig || (carry > 0 && 2ll * sh[0] >= nsig - f)) st = 2;      // DM_MOVE_OUTSIDE
        status[r] = st;
        n_stat[r] = st ? 0 : nrow;
        if (!st && nrow > 0) ev_start[e0] = (unsigned long long)f;
        sh_status = st;
    }
    __syncthreads();
    if (sh_status)
        for (long long k = tid; k < nrow; k += MOVE_THREADS) {
            ev_start[e0 + k] = 0ull;
            ev_length[e0 + k] = 0ull;
        }
}

__global__ __launch_bounds__(MOVE_THREADS) void move_write_kernel(const unsigned char* __restrict__ move, const long long* __restrict__ mv_off,
                                                                  const long long* __restrict__ chunk_off, const int n_reads, const int* __restrict__ cbase,
                                                                  const int* __restrict__ status, const long long* __restrict__ first,
                                                                  const long long* __restrict__ ev_off, unsigned long long* __restrict__ ev_start) {
    __shared__ int w_cnt[MOVE_THREADS / 64];
    const long long c = blockIdx.x;
    const int r = move_find_read(chunk_off, n_reads, c);
    if (status[r]) return;                          // (uniform: the whole workgroup belongs to one read)
    const long long t0 = mv_off[r], t1 = mv_off[r + 1];
    const long long a = (t0 & ~15ll) + (c - chunk_off[r]) * MOVE_CHUNK + threadIdx.x * 16;
    unsigned m = move_mask16(move, a, t0, t1);
    int tot;
    const int pre = move_wave_prefix(__popc(m), &tot);
    if ((threadIdx.x & 63) == 0) w_cnt[threadIdx.x >> 6] = tot;
    __syncthreads();
    long long k = (long long)cbase[c] + pre;        // number of the lane's first boundary within the read
    for (int w = 0; w < int(threadIdx.x >> 6); ++w) k += w_cnt[w];
    const long long e0 = ev_off[r], nrow = ev_off[r + 1] - e0, f = first[r];
    while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1u;
        if (k + 1 < nrow) ev_start[e0 + k + 1] = (unsigned long long)(f + 2 * (a + j - t0));
        ++k;
    }
}

__global__ void move_length_kernel(const unsigned long long* __restrict__ ev_start, const long long* __restrict__ ev_off, const long long* __restrict__ raw_off,
                                   const int* __restrict__ status, const int n_reads, const long long n_events, unsigned long long* __restrict__ ev_length) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= n_events) return;
    const int r = move_find_read(ev_off, n_reads, e);
    if (status[r]) return;                          // zeroed by move_scan_kernel
    const unsigned long long end = e + 1 < ev_off[r + 1] ? ev_start[e + 1] : (unsigned long long)(raw_off[r + 1] - raw_off[r]);
    ev_length[e] = end - ev_start[e];
}

// ---- device: the same order statistics, one workgroup per read (dm_signal_event_stats_batch) ----
// The distinct sample values of a read (a few hundred to a few thousand of the 65,536 bins) are compacted into LDS; the four
// medians are k-th elements of (key, count) lists: two of them in the natural order of the values ((x - mshift) / mscale is
// monotone in x), two after a bitonic sort by |x - m| keys computed with the host's exact float64 expressions (no
// contraction), so the results are bit-identical to norm_from_hist.  A read with more than NORM_CAP distinct values or a zero
// scale (constant signal: the host path then divides by zero like numpy) raises its fallback flag and the caller redoes the
// batch on the host path.
constexpr int NORM_CAP = 4096;
constexpr int NORM_THREADS = 256;
constexpr size_t NORM_LDS = size_t(NORM_CAP) * (4 + 4 + 8 + 4 + 4) + 2 * NORM_THREADS * 4;

__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* tmp /*[2 * NORM_THREADS]*/, unsigned& total) {
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    int in = 0;
    for (int off = 1; off < NORM_THREADS; off <<= 1) {       // Hillis-Steele, double buffered
        const int out = 1 - in;
        tmp[out * NORM_THREADS + t] = tmp[in * NORM_THREADS + t] + (t >= off ? tmp[in * NORM_THREADS + t - off] : 0u);
        __syncthreads();
        in = out;
    }
    const unsigned incl = tmp[in * NORM_THREADS + t];
    total = tmp[in * NORM_THREADS + NORM_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// inclusive prefix sums of cnt[0..n) into cum[0..n) (n <= NORM_CAP); returns the total
__device__ __forceinline__ unsigned block_prefix(const unsigned* cnt, unsigned* cum, const int n, unsigned* tmp) {
    constexpr int PER = NORM_CAP / NORM_THREADS;
    const int b = threadIdx.x * PER;
    unsigned loc = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) loc += (b + i < n) ? cnt[b + i] : 0u;
    unsigned total;
    unsigned run = block_exclusive_scan(loc, tmp, total);
#pragma unroll
    for (int i = 0; i < PER; ++i)
        if (b + i < n) {
            run += cnt[b + i];
            cum[b + i] = run;
        }
    __syncthreads();
    return total;
}

// index of the k-th element (0-based) of the multiset described by inclusive prefix sums cum[0..n)
__device__ __forceinline__ int kth_index(const unsigned* cum, const int n, const unsigned k) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ascending bitonic sort of (key, cnt) pairs, p = power of two >= the live count (padding: +inf keys, zero counts)
__device__ __forceinline__ void bitonic_sort(double* key, unsigned* cnt, const int p) {
    for (int k = 2; k <= p; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < p; i += NORM_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = (i & k) == 0;
                    const double a = key[i], b = key[ixj];
                    if ((a > b) == up && a != b) {
                        key[i] = b;
                        key[ixj] = a;
                        const unsigned c = cnt[i];
                        cnt[i] = cnt[ixj];
                        cnt[ixj] = c;
                    }
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ double median_sorted(const double* key, const unsigned* cum, const int n, const unsigned total) {
#pragma clang fp contract(off)
    const unsigned k_hi = total / 2, k_lo = (total % 2) ? k_hi : k_hi - 1;
    const double v_hi = key[kth_index(cum, n, k_hi)];
    if (total % 2) return v_hi;
    const double v_lo = key[kth_index(cum, n, k_lo)];
    return (0.0 + v_lo + v_hi) / 2.0;
}

__global__ __launch_bounds__(NORM_THREADS) void signal_norm_batch_kernel(const unsigned* __restrict__ hist /*[reads][65536]*/,
                                                                         Norm* __restrict__ norms, int* __restrict__ fallback, const int* __restrict__ vrange) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char norm_lds[];
    double* key = reinterpret_cast<double*>(norm_lds);                 // [CAP]
    int* val = reinterpret_cast<int*>(key + NORM_CAP);                 // [CAP]
    unsigned* cnt = reinterpret_cast<unsigned*>(val + NORM_CAP);       // [CAP] counts in value order
    unsigned* kcnt = cnt + NORM_CAP;                                   // [CAP] counts carried through a sort
    unsigned* cum = kcnt + NORM_CAP;                                   // [CAP]
    unsigned* tmp = cum + NORM_CAP;                                    // [2 * THREADS]
    const int r = blockIdx.x, t = threadIdx.x;
    const unsigned* h = hist + size_t(r) * 65536;
    // 1. compaction of the non-empty bins, ascending values: thread t owns the t-th piece of the bins [smallest, largest sample value of the read]
    const int bin0 = vrange[r] + 32768, bin1 = vrange[gridDim.x + r] + 32768;
    if (bin1 < bin0) {                      // (no sample at all: cannot happen for a request that passed the checks)
        if (t == 0) fallback[r] = 1;
        return;
    }
    const int BINS_PER = (bin1 - bin0 + NORM_THREADS) / NORM_THREADS;
    const int mine0 = bin0 + t * BINS_PER;
    const int mine_n = min(BINS_PER, bin1 + 1 - mine0);      // may be <= 0 for the last threads
    unsigned mine = 0;
    for (int i = 0; i < mine_n; ++i) mine += h[mine0 + i] ? 1u : 0u;
    unsigned nv;
    unsigned at = block_exclusive_scan(mine, tmp, nv);
    if (nv > unsigned(NORM_CAP) || nv == 0) {
        if (t == 0) fallback[r] = 1;
        return;
    }
    for (int i = 0; i < mine_n; ++i) {
        const unsigned c = h[mine0 + i];
        if (c) {
            val[at] = mine0 + i - 32768;
            cnt[at] = c;
            ++at;
        }
    }
    __syncthreads();
    const int n = int(nv);
    int p = 1;
    while (p < n) p <<= 1;
    // 2. mshift = median(x): natural order
    const unsigned total = block_prefix(cnt, cum, n, tmp);
    const unsigned k_hi = total / 2, k_lo = (total % 2) ? k_hi : k_hi - 1;
    const int x_hi = val[kth_index(cum, n, k_hi)], x_lo = val[kth_index(cum, n, k_lo)];
    const double mshift = (total % 2) ? (double)x_hi : (0.0 + (double)x_lo + (double)x_hi) / 2.0;
    __syncthreads();
    // 3. mscale = median(|x - mshift|)
    for (int i = t; i < p; i += NORM_THREADS) {
        key[i] = i < n ? fabs((double)val[i] - mshift) : __longlong_as_double(0x7ff0000000000000ll);
        kcnt[i] = i < n ? cnt[i] : 0u;
    }
    __syncthreads();
    bitonic_sort(key, kcnt, p);
    block_prefix(kcnt, cum, n, tmp);
    const double mscale = median_sorted(key, cum, n, total);
    __syncthreads();
    if (!(mscale > 0.0)) {                  // constant signal over the slice: the host path reproduces numpy's division by zero
        if (t == 0) fallback[r] = 1;
        return;
    }
    // 4. med = median((x - mshift) / mscale): monotone in x, so the k-th keys belong to the k-th values
    const double t_hi = ((double)x_hi - mshift) / mscale, t_lo = ((double)x_lo - mshift) / mscale;
    const double med = (total % 2) ? t_hi : (0.0 + t_lo + t_hi) / 2.0;
    // 5. mad = median(|(x - mshift) / mscale - med|)
    for (int i = t; i < p; i += NORM_THREADS) {
        key[i] = i < n ? fabs(((double)val[i] - mshift) / mscale - med) : __longlong_as_double(0x7ff0000000000000ll);
        kcnt[i] = i < n ? cnt[i] : 0u;
    }
    __syncthreads();
    bitonic_sort(key, kcnt, p);
    block_prefix(kcnt, cum, n, tmp);
    const double mad = median_sorted(key, cum, n, total);
    if (t == 0) {
        Norm o;
        o.mshift = mshift;
        o.mscale = mscale;
        o.med = med;
        o.mad = mad;
        o.lower = med - (mad * 5);
        o.upper = med + (mad * 5);
        norms[r] = o;
        fallback[r] = 0;
    }
}

// ---- host: order statistics on the histogram (numpy median semantics) ----
struct Bin {
    double key;
    unsigned long long count;
};

// median of the multiset {key_b repeated count_b}: numpy = mean of the two middle elements for even sizes
inline double median_of_bins(std::vector<Bin>& bins, const unsigned long long total) {
#pragma clang fp contract(off)
    std::sort(bins.begin(), bins.end(), [](const Bin& a, const Bin& b) { return a.key < b.key; });
    const unsigned long long k_hi = total / 2;                     // 0-based index of the upper middle
    const unsigned long long k_lo = (total % 2) ? k_hi : k_hi - 1;
    double v_lo = 0.0, v_hi = 0.0;
    unsigned long long seen = 0;
    bool have_lo = false;
    for (const Bin& b : bins) {
        const unsigned long long next = seen + b.count;
        if (!have_lo && k_lo < next) {
            v_lo = b.key;
            have_lo = true;
        }
        if (k_hi < next) {
            v_hi = b.key;
            break;
        }
        seen = next;
    }
    if (total % 2) return v_hi;
    return (0.0 + v_lo + v_hi) / 2.0;
}

inline Norm norm_from_hist(const unsigned* hist) {
#pragma clang fp contract(off)
    std::vector<int> vals;
    unsigned long long total = 0;
    for (int i = 0; i < 65536; ++i)
        if (hist[i]) {
            vals.push_back(i - 32768);
            total += hist[i];
        }
    std::vector<Bin> bins(vals.size());
    Norm p{};
    for (size_t i = 0; i < vals.size(); ++i) bins[i] = {(double)vals[i], hist[vals[i] + 32768]};
    p.mshift = median_of_bins(bins, total);
    for (size_t i = 0; i < vals.size(); ++i) bins[i] = {std::fabs((double)vals[i] - p.mshift), hist[vals[i] + 32768]};
    p.mscale = median_of_bins(bins, total);
    for (size_t i = 0; i < vals.size(); ++i) bins[i] = {((double)vals[i] - p.mshift) / p.mscale, hist[vals[i] + 32768]};
    p.med = median_of_bins(bins, total);
    for (size_t i = 0; i < vals.size(); ++i)
        bins[i] = {std::fabs(((double)vals[i] - p.mshift) / p.mscale - p.med), hist[vals[i] + 32768]};
    p.mad = median_of_bins(bins, total);
    p.lower = p.med - (p.mad * 5);
    p.upper = p.med + (p.mad * 5);
    return p;
}

}  // namespace sig

struct dm_signal {
    int device = 0;
    hipStream_t stream = nullptr;
    // The device blocks, grow-only.  A paired table (EV, OUT, FB, MVCHUNK) holds its parts back to back at a stride of the call that fills it - its own
    // event or chunk count - and every kernel takes the parts as separate pointers.
    enum {
        RAW,        // short: the samples, + RAW_SLACK
        EV,         // u64 [2][events]: start | length
        OUT,        // f32 [2][events]: mean | stdv
        HIST,       // u32 [65536], LUT f64 [65536]: the single-read call's (allocated at create)
        LUT,
        NORM,       // f64 [samples]: the single-read call's optional normalised signal
        // the per-read group of a batch (reserve_reads)
        BHIST,      // u32 [reads][65536]
        BLUT,       // f64 [reads][65536]
        BMETA,      // i64 [3][reads + 1]: lo | hi | raw_off
        BNORM,      // sig::Norm [reads]
        BFLAG,      // int [reads]: 1 = this read needs the host order statistics
        EVOFF,      // i64 [2][reads + 1]: ev_off | n_stat, the events a statistics kernel computes
        VRANGE,     // int [2][reads]: smallest | largest sample value of a read's slice
        BFULL,      // int [reads]: 1 = an event of the read reaches outside its slice, its value table is written whole
        EVREAD,     // int [events]: host-table form, the read of every event
        FB,         // f32 [2][events]: resident form, fall-back mean | stdv of the batch's events
        RFLAG,      // int: resident form, range flag of the call
        // move form: what the segmentation kernels read and write
        MOVE,       // u8: the batch's move tables, + MOVE_SLACK
        MVMETA,     // i64 [3][reads + 1]: mv_off | chunk_off | first
        MVSTATUS,   // int [reads]
        MVCHUNK,    // int [3][chunks]: count | last | base of every chunk
        N_BUF
    };
    static constexpr size_t RAW_SLACK = 8 * sizeof(short);   // bytes behind the samples that belong to the block
    static constexpr size_t MOVE_SLACK = 16;                 // the last aligned 16-byte word of a table may reach behind the tables
    DevBufs<N_BUF> b{"dm_signal"};
    std::vector<unsigned> h_hist;
    bool host_order_statistics = false;   // DEEPMOD_SIGNAL_HOST_NORM=1: always take the host path (the cross-check of the tests)
    unsigned* h_bhist = nullptr;          // page-locked, [cap_hbhist][65536]: the histograms come back by DMA
    int64_t cap_hbhist = 0;
};

namespace {

using SB = dm_signal;

int reserve_raw(dm_signal* s, int64_t n_raw) { return s->b.ensure(SB::RAW, size_t(n_raw) * sizeof(short) + SB::RAW_SLACK); }

int reserve_events(dm_signal* s, int64_t n_ev) {
    const int rc = s->b.ensure(SB::EV, size_t(n_ev) * 2 * sizeof(unsigned long long));
    return rc != DM_OK ? rc : s->b.ensure(SB::OUT, size_t(n_ev) * 2 * sizeof(float));
}

// the eight blocks of a batch that are sized by its reads
int reserve_reads(dm_signal* s, int64_t n_reads) {
    const size_t n = size_t(n_reads);
    const size_t bytes[][2] = {{SB::BHIST, n * 65536 * sizeof(unsigned)}, {SB::BLUT, n * 65536 * sizeof(double)}, {SB::BMETA, 3 * (n + 1) * sizeof(long long)},
                               {SB::BNORM, n * sizeof(sig::Norm)},        {SB::BFLAG, n * sizeof(int)},           {SB::EVOFF, 2 * (n + 1) * sizeof(long long)},
                               {SB::VRANGE, 2 * n * sizeof(int)},         {SB::BFULL, n * sizeof(int)}};
    for (const auto& e : bytes) {
        const int rc = s->b.ensure(int(e[0]), e[1]);
        if (rc != DM_OK) return rc;
    }
    return DM_OK;
}

}  // namespace

extern "C" {

dm_signal* dm_signal_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        fail(DM_EDEVICE, "dm_signal_create: no such device %d", device);
        return nullptr;
    }
    dm_signal* s = new dm_signal();
    s->device = device;
    s->h_hist.resize(65536);
    if (const char* e = std::getenv("DEEPMOD_SIGNAL_HOST_NORM")) s->host_order_statistics = e[0] == '1';
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&s->stream) != hipSuccess ||
        s->b.ensure(SB::HIST, 65536 * sizeof(unsigned)) != DM_OK || s->b.ensure(SB::LUT, 65536 * sizeof(double)) != DM_OK ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(sig::signal_hist_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, sig::LDS_COPIES * sig::LDS_BINS * 4) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(sig::signal_hist_batch_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, sig::LDS_COPIES * sig::LDS_BINS * 4) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(sig::signal_norm_batch_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, int(sig::NORM_LDS)) != hipSuccess) {
        fail(DM_EDEVICE, "dm_signal_create: device setup failed: %s", hipGetErrorString(hipGetLastError()));
        dm_signal_destroy(s);
        return nullptr;
    }
    return s;
}

void dm_signal_destroy(dm_signal* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    s->b.release();
    if (s->h_bhist) (void)hipHostFree(s->h_bhist);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int dm_signal_event_stats(dm_signal* s, const int16_t* raw, int64_t n_raw, const uint64_t* ev_start,
                          const uint64_t* ev_length, int64_t n_events, float* ev_mean, float* ev_stdv, double* norm6,
                          int64_t* first_empty, double* normalized) {
    if (!s) return fail(DM_EINVAL, "null signal handle");
    if (!raw || n_raw <= 0) return fail(DM_EINVAL, "empty raw signal");
    if (n_events <= 0 || !ev_start || !ev_length) return fail(DM_EINVAL, "no events");
    if (is_device_ptr(ev_start) || is_device_ptr(ev_length) || is_device_ptr(ev_mean) || is_device_ptr(ev_stdv))
        return fail(DM_EINVAL, "event tables are host arrays");
    HIP_TRY(hipSetDevice(s->device));
    // slice covered by the events (myDetect.py:272): [start_0, start_last + length_last), clamped like a numpy slice
    long long lo, hi;
    if (!sig::covered_slice(ev_start, ev_length, 0, n_events, n_raw, &lo, &hi)) return fail(DM_EINVAL, "events cover no signal (start %lld, end %lld, %lld samples)", lo, hi, (long long)n_raw);

    int rc;
    const short* d_raw = reinterpret_cast<const short*>(raw);
    if (!is_device_ptr(raw)) {
        if ((rc = reserve_raw(s, n_raw)) != DM_OK) return rc;
        HIP_TRY(hipMemcpyAsync(s->b.buf[SB::RAW], raw, size_t(n_raw) * sizeof(short), hipMemcpyHostToDevice, s->stream));
        d_raw = s->b.ptr<short>(SB::RAW);
    } else if ((reinterpret_cast<size_t>(raw) & 15) != 0) {
        return fail(DM_EINVAL, "device raw signal must be 16-byte aligned");
    }
    if ((rc = reserve_events(s, n_events)) != DM_OK) return rc;
    unsigned long long* d_start = s->b.ptr<unsigned long long>(SB::EV);
    unsigned long long* d_length = d_start + n_events;
    float* d_mean = s->b.ptr<float>(SB::OUT);
    float* d_stdv = d_mean + n_events;
    unsigned* d_hist = s->b.ptr<unsigned>(SB::HIST);
    double* d_lut = s->b.ptr<double>(SB::LUT);
    HIP_TRY(hipMemcpyAsync(d_start, ev_start, size_t(n_events) * 8, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(d_length, ev_length, size_t(n_events) * 8, hipMemcpyHostToDevice, s->stream));

    // 1. histogram of the covered slice
    HIP_TRY(hipMemsetAsync(d_hist, 0, 65536 * sizeof(unsigned), s->stream));
    {
        const long long groups = (hi - lo + 7) / 8;
        int grid = int(std::min<long long>(256, (groups + 255) / 256));
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL(sig::signal_hist_kernel, dim3(grid), dim3(256), sig::LDS_COPIES * sig::LDS_BINS * 4, s->stream, d_raw, lo, hi, d_hist);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(s->h_hist.data(), d_hist, 65536 * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    // 2. order statistics
    const sig::Norm p = sig::norm_from_hist(s->h_hist.data());
    if (norm6) {
        norm6[0] = p.mshift;
        norm6[1] = p.mscale;
        norm6[2] = p.med;
        norm6[3] = p.mad;
        norm6[4] = p.lower;
        norm6[5] = p.upper;
    }
    // 3. value table, 4. per-event statistics
    hipLaunchKernelGGL(sig::signal_lut_kernel, dim3(256), dim3(256), 0, s->stream, d_lut, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sig::event_stats_kernel, dim3(unsigned((n_events + 255) / 256)), dim3(256), 0, s->stream, d_raw,
                       (long long)n_raw, d_lut, d_start, d_length, (long long)n_events, d_mean, d_stdv);
    HIP_TRY(hipGetLastError());
    if (ev_mean) HIP_TRY(hipMemcpyAsync(ev_mean, d_mean, size_t(n_events) * 4, hipMemcpyDeviceToHost, s->stream));
    if (ev_stdv) HIP_TRY(hipMemcpyAsync(ev_stdv, d_stdv, size_t(n_events) * 4, hipMemcpyDeviceToHost, s->stream));
    if (normalized) {   // the whole normalised signal (the reference keeps it in f5data; nothing downstream reads it)
        double* dst = normalized;
        if (!is_device_ptr(normalized)) {
            if ((rc = s->b.ensure(SB::NORM, size_t(n_raw) * sizeof(double))) != DM_OK) return rc;
            dst = s->b.ptr<double>(SB::NORM);
        }
        hipLaunchKernelGGL(sig::signal_gather_kernel, dim3(512), dim3(256), 0, s->stream, d_raw, (long long)n_raw, d_lut, dst);
        HIP_TRY(hipGetLastError());
        if (dst != normalized)
            HIP_TRY(hipMemcpyAsync(normalized, dst, size_t(n_raw) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (first_empty) *first_empty = sig::first_empty_event(ev_start, ev_length, 0, n_events, n_raw);
    return DM_OK;
}

}  // extern "C"

// ---- many reads per call ----
// The reads' samples back to back in `raw` (read r = raw[raw_off[r] .. raw_off[r+1])), their event tables back to back (events of read r =
// [ev_off[r], ev_off[r+1]), starts relative to the read's first sample).  One upload, one histogram launch (blockIdx.y = read), one order-statistics
// launch (one workgroup per read), one table launch, one statistics launch over all events, one download, ONE host wait: a typical 120 k-sample read
// costs 0.15 ms in launches and waits when it travels alone.  Same kernels' arithmetic as dm_signal_event_stats: results are bit-identical to
// per-read calls.  Three forms behind one sequence of stages (signal_batch_impl):
//   host tables   dm_signal_event_stats_batch   event tables in, mean | stdv | first_empty out;
//   resident      dm_signal_event_stats_device  the statistics stay on the device (d_ev3); first_empty is an INPUT (dm_signal_plan_batch);
//   move tables   dm_signal_move_stats_device   resident, and the event tables are cut on the device from the move tables.
namespace {

// the inputs and outputs of one batched call; a pointer its form does not have is null
struct BatchCall {
    int64_t n_reads;
    const int16_t* raw;
    const int64_t* raw_off;
    const int64_t* ev_off;
    double* norm6;                           // out, optional
    const uint64_t* ev_start = nullptr;      // event forms
    const uint64_t* ev_length = nullptr;
    float* ev_mean = nullptr;                // host-table form: out, optional
    float* ev_stdv = nullptr;
    int64_t* first_empty_out = nullptr;
    float* d_ev3 = nullptr;                  // resident forms: out, a device block of the caller
    int32_t* flags = nullptr;                // out, optional
    const int64_t* first_empty = nullptr;    // resident event form
    const float* fb_mean = nullptr;
    const float* fb_stdv = nullptr;
    bool from_moves = false;                 // move form
    const uint8_t* move = nullptr;
    const int64_t* mv_off = nullptr;
    const int64_t* first = nullptr;
    int32_t* status = nullptr;               // out, [n_reads]
    bool resident() const { return d_ev3 != nullptr; }
    bool with_fb() const { return resident() && fb_mean && fb_stdv; }
};

// a call on its way through the stages: its plan, where the plan's tables lie on the device (batch_reserve), and what the downloads write into
struct BatchRun {
    const BatchCall& c;
    sig::BatchPlan p;
    short* raw = nullptr;
    unsigned long long *start = nullptr, *length = nullptr;
    float *mean = nullptr, *stdv = nullptr, *fb_mean = nullptr, *fb_stdv = nullptr;
    long long *lo = nullptr, *hi = nullptr, *off = nullptr, *ev_off = nullptr, *n_stat = nullptr;
    unsigned* hist = nullptr;
    double* lut = nullptr;
    sig::Norm* norm = nullptr;
    int *flag = nullptr, *vrange = nullptr, *full = nullptr, *ev_read = nullptr, *rflag = nullptr;
    unsigned char* move = nullptr;
    long long *mv_off = nullptr, *chunk_off = nullptr, *first = nullptr;
    int *mv_status = nullptr, *ccnt = nullptr, *clast = nullptr, *cbase = nullptr;
    std::vector<sig::Norm> h_norm;
    std::vector<int> h_flag, h_status;
    int h_rflag = 0;
};

int batch_reserve(dm_signal* s, BatchRun& q) {
    const BatchCall& c = q.c;
    const sig::BatchPlan& p = q.p;
    DevBufs<SB::N_BUF>& b = s->b;
    const size_t n = size_t(p.n_reads), n_ev = size_t(p.n_ev), n_chunks = size_t(p.n_chunks);
    int rc;
    if ((rc = reserve_raw(s, p.n_raw)) != DM_OK || (rc = reserve_events(s, p.n_ev)) != DM_OK) return rc;
    if (!c.resident() && (rc = b.ensure(SB::EVREAD, n_ev * sizeof(int))) != DM_OK) return rc;
    if ((rc = reserve_reads(s, p.n_reads)) != DM_OK) return rc;
    if (c.with_fb() && (rc = b.ensure(SB::FB, n_ev * 2 * sizeof(float))) != DM_OK) return rc;
    if (c.resident() && (rc = b.ensure(SB::RFLAG, sizeof(int))) != DM_OK) return rc;
    if (c.from_moves) {
        if ((rc = b.ensure(SB::MOVE, size_t(p.n_mv) + SB::MOVE_SLACK)) != DM_OK || (rc = b.ensure(SB::MVMETA, 3 * (n + 1) * sizeof(long long))) != DM_OK ||
            (rc = b.ensure(SB::MVSTATUS, n * sizeof(int))) != DM_OK || (rc = b.ensure(SB::MVCHUNK, 3 * n_chunks * sizeof(int))) != DM_OK)
            return rc;
        q.move = b.ptr<unsigned char>(SB::MOVE);
        q.mv_off = b.ptr<long long>(SB::MVMETA);
        q.chunk_off = q.mv_off + (n + 1);
        q.first = q.mv_off + 2 * (n + 1);
        q.mv_status = b.ptr<int>(SB::MVSTATUS);
        q.ccnt = b.ptr<int>(SB::MVCHUNK);
        q.clast = q.ccnt + n_chunks;
        q.cbase = q.ccnt + 2 * n_chunks;
    }
    q.raw = b.ptr<short>(SB::RAW);
    q.start = b.ptr<unsigned long long>(SB::EV);
    q.length = q.start + n_ev;
    q.mean = b.ptr<float>(SB::OUT);
    q.stdv = q.mean + n_ev;
    q.ev_read = b.ptr<int>(SB::EVREAD);
    if (c.with_fb()) {
        q.fb_mean = b.ptr<float>(SB::FB);
        q.fb_stdv = q.fb_mean + n_ev;
    }
    q.rflag = b.ptr<int>(SB::RFLAG);
    q.lo = b.ptr<long long>(SB::BMETA);
    q.hi = q.lo + (n + 1);
    q.off = q.lo + 2 * (n + 1);
    q.ev_off = b.ptr<long long>(SB::EVOFF);
    q.n_stat = q.ev_off + (n + 1);
    q.hist = b.ptr<unsigned>(SB::BHIST);
    q.lut = b.ptr<double>(SB::BLUT);
    q.norm = b.ptr<sig::Norm>(SB::BNORM);
    q.flag = b.ptr<int>(SB::BFLAG);
    q.vrange = b.ptr<int>(SB::VRANGE);
    q.full = b.ptr<int>(SB::BFULL);
    return DM_OK;
}

int batch_upload(dm_signal* s, BatchRun& q) {
    const BatchCall& c = q.c;
    sig::BatchPlan& p = q.p;
    const size_t n_ev = size_t(p.n_ev);
    HIP_TRY(hipMemcpyAsync(q.raw, c.raw, size_t(p.n_raw) * sizeof(short), hipMemcpyHostToDevice, s->stream));
    if (!c.from_moves) {
        HIP_TRY(hipMemcpyAsync(q.start, c.ev_start, n_ev * 8, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(q.length, c.ev_length, n_ev * 8, hipMemcpyHostToDevice, s->stream));
    }
    if (!c.resident()) HIP_TRY(hipMemcpyAsync(q.ev_read, p.ev_read.data(), n_ev * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(q.lo, p.meta.data(), p.meta.size() * sizeof(long long), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(q.ev_off, p.evmeta.data(), p.evmeta.size() * sizeof(long long), hipMemcpyHostToDevice, s->stream));
    if (c.resident()) {
        HIP_TRY(hipMemsetAsync(q.rflag, 0, sizeof(int), s->stream));
        if (c.with_fb()) {
            HIP_TRY(hipMemcpyAsync(q.fb_mean, c.fb_mean, n_ev * 4, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(q.fb_stdv, c.fb_stdv, n_ev * 4, hipMemcpyHostToDevice, s->stream));
        }
    }
    if (c.from_moves) {
        if (p.n_mv > 0) HIP_TRY(hipMemcpyAsync(q.move, c.move, size_t(p.n_mv), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(q.mv_off, p.mvmeta.data(), p.mvmeta.size() * sizeof(long long), hipMemcpyHostToDevice, s->stream));
    }
    return DM_OK;
}

// move form: the event tables from the move tables (behind the uploads on the same stream; no host wait before the statistics).  The statuses come
// back behind the statistics kernels, next to the range flag (batch_tables_and_stats): a download enqueued here would make the host wait for the
// segmentation before it launches them.
int batch_segment(dm_signal* s, BatchRun& q) {
    const int n_reads = int(q.p.n_reads);
    const unsigned n_chunks = unsigned(q.p.n_chunks);
    const long long n_ev = q.p.n_ev;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(sig::move_count_kernel, dim3(n_chunks), dim3(sig::MOVE_THREADS), 0, s->stream, q.move, q.mv_off, q.chunk_off, n_reads, q.ccnt, q.clast);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sig::move_scan_kernel, dim3(unsigned(n_reads)), dim3(sig::MOVE_THREADS), 0, s->stream, q.ccnt, q.clast, q.chunk_off, q.first, q.off,
                       q.ev_off, q.cbase, q.mv_status, q.n_stat, q.start, q.length);
    HIP_TRY(hipGetLastError());
    if (n_chunks > 0) {
        hipLaunchKernelGGL(sig::move_write_kernel, dim3(n_chunks), dim3(sig::MOVE_THREADS), 0, s->stream, q.move, q.mv_off, q.chunk_off, n_reads, q.cbase,
                           q.mv_status, q.first, q.ev_off, q.start);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sig::move_length_kernel, dim3(unsigned((n_ev + 255) / 256)), dim3(256), 0, s->stream, q.start, q.ev_off, q.off, q.mv_status, n_reads, n_ev,
                       q.length);
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

// 1. histograms of all reads, and the reads whose value table the events need whole
int batch_histograms(dm_signal* s, BatchRun& q) {
    const size_t n = size_t(q.p.n_reads);
    const long long n_ev = q.p.n_ev;
    HIP_TRY(hipMemsetAsync(q.hist, 0, n * 65536 * sizeof(unsigned), s->stream));
    // value range of every read: the minima start at 0x7f7f7f7f, the maxima at 0x80808080 (byte fills: larger / smaller than any int16)
    HIP_TRY(hipMemsetAsync(q.vrange, 0x7f, n * sizeof(int), s->stream));
    HIP_TRY(hipMemsetAsync(q.vrange + n, 0x80, n * sizeof(int), s->stream));
    // a workgroup zeroes and flushes 128 KB of privatised bins whatever it counts: one per 32,768 samples of an average read (round 5: one per 2,048 -
    // the fixed cost was 40x the samples' own bytes and the flush atomics of twenty workgroups per read met on the same few hundred bins)
    const long long avg = q.p.n_raw / q.p.n_reads;
    int gx = int(std::min<long long>(64, (avg + 32767) / 32768));
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(sig::signal_hist_batch_kernel, dim3(gx, unsigned(n)), dim3(256), sig::LDS_COPIES * sig::LDS_BINS * 4, s->stream, q.raw, q.lo, q.hi, q.hist,
                       q.vrange);
    HIP_TRY(hipGetLastError());
    // an event outside the covered slice: a pass over the event tables on the device, 16 B per event
    HIP_TRY(hipMemsetAsync(q.full, 0, n * sizeof(int), s->stream));
    hipLaunchKernelGGL(sig::event_reach_batch_kernel, dim3(unsigned((n_ev + 255) / 256)), dim3(256), 0, s->stream, q.start, q.length, q.ev_off, q.n_stat, q.lo, q.hi,
                       q.off, int(n), n_ev, q.full);
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

// 2. order statistics of all reads on the device: one stream with the tables and the statistics behind it, no host round trip
int batch_normalise_device(dm_signal* s, BatchRun& q) {
    hipLaunchKernelGGL(sig::signal_norm_batch_kernel, dim3(unsigned(q.p.n_reads)), dim3(sig::NORM_THREADS), sig::NORM_LDS, s->stream, q.hist, q.norm, q.flag,
                       q.vrange);
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

// 3. value tables, 4. statistics of all events, and the downloads of what they wrote
int batch_tables_and_stats(dm_signal* s, BatchRun& q) {
    const BatchCall& c = q.c;
    const size_t n = size_t(q.p.n_reads);
    const long long n_ev = q.p.n_ev;
    hipLaunchKernelGGL(sig::signal_lut_batch_kernel, dim3(256, unsigned(n)), dim3(256), 0, s->stream, q.lut, q.norm, q.vrange, q.full);
    HIP_TRY(hipGetLastError());
    if (c.resident()) {
        hipLaunchKernelGGL(sig::event_ev3_batch_kernel, dim3(unsigned((n_ev + 255) / 256)), dim3(256), 0, s->stream, q.raw, q.off, q.lut, q.start, q.length, q.ev_off,
                           q.n_stat, int(n), n_ev, q.fb_mean, q.fb_stdv, c.d_ev3, q.rflag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&q.h_rflag, q.rflag, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        if (c.from_moves) HIP_TRY(hipMemcpyAsync(q.h_status.data(), q.mv_status, n * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        return DM_OK;
    }
    hipLaunchKernelGGL(sig::event_stats_batch_kernel, dim3(unsigned((n_ev + 255) / 256)), dim3(256), 0, s->stream, q.raw, q.off, q.lut, q.start, q.length, q.ev_read,
                       n_ev, q.mean, q.stdv);
    HIP_TRY(hipGetLastError());
    if (c.ev_mean) HIP_TRY(hipMemcpyAsync(c.ev_mean, q.mean, size_t(n_ev) * 4, hipMemcpyDeviceToHost, s->stream));
    if (c.ev_stdv) HIP_TRY(hipMemcpyAsync(c.ev_stdv, q.stdv, size_t(n_ev) * 4, hipMemcpyDeviceToHost, s->stream));
    return DM_OK;
}

// the one host wait of the device path; *host_path: a read the kernel handed back (> NORM_CAP distinct values or a zero scale: rare)
int batch_wait_device(dm_signal* s, BatchRun& q, bool* host_path) {
    const size_t n = size_t(q.p.n_reads);
    if (q.c.norm6 || !q.c.resident()) HIP_TRY(hipMemcpyAsync(q.h_norm.data(), q.norm, n * sizeof(sig::Norm), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(q.h_flag.data(), q.flag, n * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (size_t r = 0; r < n; ++r) *host_path |= q.h_flag[r] != 0;
    return DM_OK;
}

// the host fall-back of 2.: the histograms come back (page-locked), exact order statistics on the host, their results go up for the same two kernels
int batch_normalise_host(dm_signal* s, BatchRun& q) {
    const int64_t n_reads = q.p.n_reads;
    if (s->cap_hbhist < n_reads) {
        if (s->h_bhist) (void)hipHostFree(s->h_bhist);
        s->h_bhist = nullptr;
        s->cap_hbhist = 0;
        const int64_t cap = n_reads + (n_reads >> 1);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->h_bhist), size_t(cap) * 65536 * sizeof(unsigned), hipHostMallocDefault));
        s->cap_hbhist = cap;
    }
    HIP_TRY(hipMemcpyAsync(s->h_bhist, q.hist, size_t(n_reads) * 65536 * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    {
        const int nthr = int(std::min<int64_t>(4, n_reads / 4 + 1));
        auto work = [&](int t) {
            for (int64_t r = t; r < n_reads; r += nthr) q.h_norm[r] = sig::norm_from_hist(s->h_bhist + size_t(r) * 65536);
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < nthr; ++t) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    HIP_TRY(hipMemcpyAsync(q.norm, q.h_norm.data(), size_t(n_reads) * sizeof(sig::Norm), hipMemcpyHostToDevice, s->stream));
    if (q.c.resident()) HIP_TRY(hipMemsetAsync(q.rflag, 0, sizeof(int), s->stream));
    return DM_OK;
}

// after the last host wait: what the call returns in host arrays that no download wrote
void batch_copy_out(const BatchRun& q) {
    const BatchCall& c = q.c;
    const int64_t n_reads = q.p.n_reads;
    if (c.flags) *c.flags = q.h_rflag ? 1 : 0;
    if (c.from_moves)
        for (int64_t r = 0; r < n_reads; ++r) c.status[r] = q.h_status[r];
    if (c.norm6)
        for (int64_t r = 0; r < n_reads; ++r) {
            const sig::Norm& v = q.h_norm[r];
            double* o = c.norm6 + 6 * r;
            o[0] = v.mshift; o[1] = v.mscale; o[2] = v.med; o[3] = v.mad; o[4] = v.lower; o[5] = v.upper;
        }
    if (c.first_empty_out)
        for (int64_t r = 0; r < n_reads; ++r)
            c.first_empty_out[r] = sig::first_empty_event(c.ev_start, c.ev_length, c.ev_off[r], c.ev_off[r + 1], c.raw_off[r + 1] - c.raw_off[r]);
}

int signal_batch_impl(dm_signal* s, const BatchCall& c) {
    if (!s) return fail(DM_EINVAL, "null signal handle");
    if (c.n_reads > 0) {     // the arrays the plan does not look at, and what only this half can tell; every other check is the plan's (signalplan.inc)
        if (!c.raw || (c.from_moves && (!c.move || !c.status))) return fail(DM_EINVAL, "null input");
        if (is_device_ptr(c.raw) || is_device_ptr(c.ev_start) || is_device_ptr(c.ev_mean) || is_device_ptr(c.move)) return fail(DM_EINVAL, "the batched call takes host arrays");
        if (c.resident() && ((!c.first_empty && !c.from_moves) || !is_device_ptr(c.d_ev3)))
            return fail(DM_EINVAL, "the resident form takes first_empty (dm_signal_plan_batch) and a device block");
    }
    BatchRun q{c};
    int rc = c.from_moves ? sig::plan_moves(q.p, c.n_reads, c.raw_off, c.ev_off, c.mv_off, c.first)
                          : sig::plan_events(q.p, c.n_reads, c.raw_off, c.ev_off, c.ev_start, c.ev_length, c.resident(), c.first_empty, c.with_fb());
    if (rc != DM_OK || c.n_reads == 0) return rc;
    HIP_TRY(hipSetDevice(s->device));
    q.h_norm.resize(size_t(c.n_reads));
    q.h_flag.assign(size_t(c.n_reads), 0);
    q.h_status.assign(c.from_moves ? size_t(c.n_reads) : 0, 0);
    if ((rc = batch_reserve(s, q)) != DM_OK || (rc = batch_upload(s, q)) != DM_OK) return rc;
    if (c.from_moves && (rc = batch_segment(s, q)) != DM_OK) return rc;
    if ((rc = batch_histograms(s, q)) != DM_OK) return rc;
    bool host_path = s->host_order_statistics;
    if (!host_path && ((rc = batch_normalise_device(s, q)) != DM_OK || (rc = batch_tables_and_stats(s, q)) != DM_OK || (rc = batch_wait_device(s, q, &host_path)) != DM_OK))
        return rc;
    if (host_path) {
        if ((rc = batch_normalise_host(s, q)) != DM_OK || (rc = batch_tables_and_stats(s, q)) != DM_OK) return rc;
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    batch_copy_out(q);
    return DM_OK;
}

}  // namespace

extern "C" {

int dm_signal_event_stats_batch(dm_signal* s, int64_t n_reads, const int16_t* raw, const int64_t* raw_off, const uint64_t* ev_start,
                                const uint64_t* ev_length, const int64_t* ev_off, float* ev_mean, float* ev_stdv, double* norm6,
                                int64_t* first_empty) {
    BatchCall c{n_reads, raw, raw_off, ev_off, norm6};
    c.ev_start = ev_start;
    c.ev_length = ev_length;
    c.ev_mean = ev_mean;
    c.ev_stdv = ev_stdv;
    c.first_empty_out = first_empty;
    return signal_batch_impl(s, c);
}

// The RESIDENT form (round 6): the same four kernels, but the per-event statistics never leave the device - d_ev3 [n_events][3] (a device block of the
// caller, written on the handle's stream and complete when the call returns) takes (mean, stdv, length) of every merged event of the batch, the table's
// fall-back values (fb_mean / fb_stdv [n_events], host, needed only when some read has an empty event) already merged; dm_rows_assemble reads them in place
// (dm_rows_emit_resident's descriptors index this block).  Host arrays should be page-locked (dm_host_alloc): the uploads then overlap whatever else
// the device does.  first_empty [n_reads]: INPUT, from dm_signal_plan_batch.  flags (optional): bit 0 = a mean or stdv the call computed is outside the split-f16 kernels' range (lengths and fall-back values: dm_rows_emit_resident's in_range, for the events rows show).
int dm_signal_event_stats_device(dm_signal* s, int64_t n_reads, const int16_t* raw, const int64_t* raw_off, const uint64_t* ev_start,
                                 const uint64_t* ev_length, const int64_t* ev_off, const int64_t* first_empty, const float* fb_mean, const float* fb_stdv,
                                 float* d_ev3, double* norm6, int32_t* flags) {
    if (!d_ev3) return fail(DM_EINVAL, "dm_signal_event_stats_device: null device block");
    BatchCall c{n_reads, raw, raw_off, ev_off, norm6};
    c.ev_start = ev_start;
    c.ev_length = ev_length;
    c.d_ev3 = d_ev3;
    c.flags = flags;
    c.first_empty = first_empty;
    c.fb_mean = fb_mean;
    c.fb_stdv = fb_stdv;
    return signal_batch_impl(s, c);
}

// The resident form for reads with move tables (detect --move): see include/deepmod_hip.h.  The segmentation kernels (sig::move_*_kernel) write the
// handle's event tables, the statistics kernels above run unchanged.  No fall-back values: every event of a read that passes is non-empty
// (first_empty == its event count), and a read that fails shows no statistics.
int dm_signal_move_stats_device(dm_signal* s, int64_t n_reads, const int16_t* raw, const int64_t* raw_off, const uint8_t* move, const int64_t* mv_off,
                                const int64_t* first, const int64_t* ev_off, float* d_ev3, int32_t* status, double* norm6, int32_t* flags) {
    if (!d_ev3) return fail(DM_EINVAL, "dm_signal_move_stats_device: null device block");
    BatchCall c{n_reads, raw, raw_off, ev_off, norm6};
    c.d_ev3 = d_ev3;
    c.flags = flags;
    c.from_moves = true;
    c.move = move;
    c.mv_off = mv_off;
    c.first = first;
    c.status = status;
    return signal_batch_impl(s, c);
}

}  // extern "C"

