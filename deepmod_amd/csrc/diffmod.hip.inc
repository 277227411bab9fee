// diffmod.hip.inc — `diffmod`, the kernels (part of offline.hip through diffmod.inc, which states the fate of a key and Fisher's exact test and holds
// the handle).  One run joins the sample's and the controls' counters (dm_summary tables: touch | cov | mod, `length` ints each) and tests every key
// that is deep enough in both.
//   select_kernel<WRITE>     a workgroup takes tiles of dfk::TILE_POS positions (grid-stride over the tiles, at most MAX_BLOCKS workgroups); lane i
//                            reads position tile + i + 256 k of the eight cov / mod columns (every load of a wave is one run of 256 bytes) and applies
//                            dfk::fate.  Launched twice: <false> counts - the four counters of either strand as mo_count_kernel reduces its own, and
//                            the tested keys of every tile; <true>, after scan_kernel has turned those into offsets, writes the tested keys with
//                            their four counts into the work list in key order (ascending position, '+' before '-'; a block scan per slab of 256
//                            positions) and appends the index of every key with more than SMALL_S tables to the list of large keys.
//   fisher_kernel<LARGE>     <true>: a workgroup per large key, grid-stride over their list; lane i sums the tables lo + i, lo + i + 256, .., the
//                            lanes are reduced by shuffles, the four waves in LDS in wave order.  <false>: a workgroup per chunk of CHUNK work items,
//                            a group of 16 lanes per key; lane j of the group sums the tables lo + j, lo + j + 16, .. (16 at most), the group is
//                            reduced by shuffles; the p of a large key is read as the launch before left it.  Writes p per work item, adds every
//                            key to the p histogram (32-bit LDS atomics, flushed with 64-bit global ones) and counts the chunk's keys with
//                            p <= alpha.  Per table: four gathers from lf beyond the key's five constants, one fp64 exp.
//   records_kernel           after scan_kernel over the chunks' counts: the work items with p <= alpha into the record arrays, in key order.
//   scan_kernel              one workgroup: exclusive scan of n 32-bit counts into 64-bit offsets, and their sum.
// Determinism: which lane sums which tables, and the order of every reduction, depend on the key alone, so two runs give the same bits; the
// order in which the indices of large keys land in their list does not reach any result (p is written by work index).
// Bounds: a table index is < length; a work index is < n_work and a record index < n_records by the scans (and checked again before every
// store); an lf index is in [0, cA + cB] (diffmod.inc), at most MAX_TOTAL for a tested key.  Only vector stores and atomics; no inline assembly.
#pragma once
#include "host.h"
#include "blockscan.hip.inc"
#define DM_DIFFMOD_RULE_ONLY
#include "diffmod.inc"
#undef DM_DIFFMOD_RULE_ONLY

namespace dfk {

constexpr int THREADS = 256;
constexpr int TILE_POS = 1024;                      // positions of one tile of the sweep (dm_diffmod_tile_positions)
constexpr int PER_LANE = TILE_POS / THREADS;        // positions of a tile per lane, THREADS apart
constexpr int MAX_BLOCKS = 2048;
constexpr int GROUP = 16;                           // lanes that share a small key
constexpr int SMALL_S = 256;                        // tables of a small key at most: 16 per lane of its group (dm_diffmod_small_support)
constexpr int CHUNK = THREADS;                      // work items per workgroup of fisher_kernel<false> and records_kernel
constexpr int LARGE_BLOCKS = 1024;
enum { W_WORK = 2 * N_COUNT, W_LARGE, W_RECORDS, N_WORDS };          // the 64-bit words of a run: the counters [2][N_COUNT], then three lengths

struct WorkList {
    unsigned* key;                                  // 2 position + strand
    int *cA, *mA, *cB, *mB;
    double* p;
    unsigned* large;                                // work indices of the keys with more than SMALL_S tables, in no particular order
    long long n;
};

struct Records {
    int* pos;
    unsigned char* strand;
    int *cA, *mA, *cB, *mB;
    double* p;
    long long n;
};

template <bool WRITE>
__global__ __launch_bounds__(THREADS) void select_kernel(const long long length, const int* __restrict__ plus, const int* __restrict__ minus,
                                                        const int* __restrict__ ctrl_plus, const int* __restrict__ ctrl_minus, const int cov, int* __restrict__ tile_n,
                                                        const long long* __restrict__ tile_off, const WorkList w, unsigned long long* __restrict__ counts) {
    __shared__ long long wave_total[THREADS / 64];
    __shared__ long long part[THREADS / 64][2 * N_COUNT];
    const int lane = threadIdx.x & 63;
    unsigned n[2 * N_COUNT];
#pragma unroll
    for (int k = 0; k < 2 * N_COUNT; ++k) n[k] = 0u;
    const long long tiles = (length + TILE_POS - 1) / TILE_POS;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long q0 = tile * TILE_POS;
        long long base = WRITE ? tile_off[tile] : 0;
        for (int k = 0; k < PER_LANE; ++k) {                          // the whole workgroup iterates together: block_exclusive_scan has barriers
            const long long p = q0 + (long long)k * THREADS + threadIdx.x;
            const bool in = p < length;
            int cv[2] = {0, 0}, md[2] = {0, 0}, ccv[2] = {0, 0}, cmd[2] = {0, 0};
            if (in) {
                cv[0] = plus[length + p];
                md[0] = plus[2 * length + p];
                cv[1] = minus[length + p];
                md[1] = minus[2 * length + p];
                ccv[0] = ctrl_plus[length + p];
                cmd[0] = ctrl_plus[2 * length + p];
                ccv[1] = ctrl_minus[length + p];
                cmd[1] = ctrl_minus[2 * length + p];
            }
            int f[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f[s] = in ? fate(cov, cv[s], ccv[s]) : int(F_IGNORED);
                if (!WRITE) {
#pragma unroll
                    for (int j = 0; j < N_COUNT; ++j) n[s * N_COUNT + j] += f[s] == j ? 1u : 0u;
                }
            }
            long long total;
            const long long before = csites::block_exclusive_scan<THREADS>((f[0] == F_TESTED ? 1 : 0) + (f[1] == F_TESTED ? 1 : 0), wave_total, total);
            if (WRITE) {
                long long at = base + before;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (f[s] != F_TESTED) continue;
                    if (at < w.n) {
                        const int ma = held(md[s], cv[s]), mb = held(cmd[s], ccv[s]);
                        w.key[at] = 2u * unsigned(p) + unsigned(s);
                        w.cA[at] = cv[s];
                        w.mA[at] = ma;
                        w.cB[at] = ccv[s];
                        w.mB[at] = mb;
                        int lo;
                        if (support(cv[s], ma, ccv[s], mb, lo) > SMALL_S) {
                            const unsigned long long slot = atomicAdd(&counts[W_LARGE], 1ull);
                            if (slot < (unsigned long long)w.n) w.large[slot] = unsigned(at);
                        }
                    }
                    ++at;
                }
            }
            base += total;
        }
        if (!WRITE && threadIdx.x == 0) tile_n[tile] = int(base);    // at most 2 TILE_POS
    }
    if (WRITE) return;
#pragma unroll
    for (int k = 0; k < 2 * N_COUNT; ++k) {
        long long v = n[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2 * N_COUNT) {
        long long v = 0;
#pragma unroll
        for (int wv = 0; wv < THREADS / 64; ++wv) v += part[wv][threadIdx.x];
        if (v != 0) atomicAdd(counts + threadIdx.x, (unsigned long long)v);
    }
}

// off[i] = counts[0] + .. + counts[i - 1], *sum = all of them.  One workgroup.
__global__ __launch_bounds__(THREADS) void scan_kernel(const int* __restrict__ counts, const long long n, long long* __restrict__ off, unsigned long long* __restrict__ sum) {
    __shared__ long long wave_total[THREADS / 64];
    long long carry = 0;
    for (long long first = 0; first < n; first += THREADS) {
        const long long i = first + threadIdx.x;
        long long total;
        const long long before = csites::block_exclusive_scan<THREADS>(i < n ? counts[i] : 0, wave_total, total);
        if (i < n) off[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) *sum = (unsigned long long)carry;
}

template <bool LARGE>
__global__ __launch_bounds__(THREADS) void fisher_kernel(const double* __restrict__ lf, const WorkList w, const double alpha, int* __restrict__ chunk_n,
                                                        unsigned long long* __restrict__ hist, const unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (LARGE) {
        __shared__ double wave_sum[THREADS / 64];
        const unsigned long long listed = counts[W_LARGE];
        const long long n_large = listed < (unsigned long long)w.n ? (long long)listed : w.n;
        for (long long i = blockIdx.x; i < n_large; i += gridDim.x) {                  // (the workgroup iterates together)
            const long long idx = w.large[i];
            if (idx >= w.n) continue;
            const int cA = w.cA[idx], mA = w.mA[idx], cB = w.cB[idx], mB = w.mB[idx], M = mA + mB;
            int lo;
            const int S = support(cA, mA, cB, mB, lo);
            const double cut = log_term(lf, cA, cB, M, mA) + TIE;
            double sum = 0.0;
            int x = lo + int(threadIdx.x);
            for (; x + 3 * THREADS < lo + S; x += 4 * THREADS) {      // four tables' gathers in flight; the terms are added in the order of x all the same
                const double L0 = log_term(lf, cA, cB, M, x), L1 = log_term(lf, cA, cB, M, x + THREADS), L2 = log_term(lf, cA, cB, M, x + 2 * THREADS),
                             L3 = log_term(lf, cA, cB, M, x + 3 * THREADS);
                sum += L0 <= cut ? ::exp(L0) : 0.0;
                sum += L1 <= cut ? ::exp(L1) : 0.0;
                sum += L2 <= cut ? ::exp(L2) : 0.0;
                sum += L3 <= cut ? ::exp(L3) : 0.0;
            }
            for (; x < lo + S; x += THREADS) sum += term(lf, cA, cB, M, x, cut);
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
            if (lane == 0) wave_sum[wave] = sum;
            __syncthreads();
            if (threadIdx.x == 0) {
                double all = wave_sum[0];
#pragma unroll
                for (int k = 1; k < THREADS / 64; ++k) all += wave_sum[k];
                w.p[idx] = capped(all);
            }
            __syncthreads();                                          // wave_sum may be written again
        }
    } else {
        __shared__ unsigned lds_hist[HIST_BINS];
        __shared__ int wave_pass[THREADS / 64];
        if (threadIdx.x < HIST_BINS) lds_hist[threadIdx.x] = 0u;
        __syncthreads();
        const int j = threadIdx.x & (GROUP - 1), g = threadIdx.x / GROUP;
        const long long first = (long long)blockIdx.x * CHUNK;
        int passed = 0;
        for (int it = 0; it < CHUNK / (THREADS / GROUP); ++it) {      // whole waves iterate together: the shuffles below see all 64 lanes
            const long long idx = first + it * (THREADS / GROUP) + g;
            const bool have = idx < w.n;
            int cA = 0, mA = 0, cB = 0, mB = 0, lo = 0, S = 0;
            if (have) {
                cA = w.cA[idx], mA = w.mA[idx], cB = w.cB[idx], mB = w.mB[idx];
                S = support(cA, mA, cB, mB, lo);
            }
            const bool small = have && S > 1 && S <= SMALL_S;
            double sum = 0.0;
            if (small) {
                const int M = mA + mB;
                const double cut = log_term(lf, cA, cB, M, mA) + TIE;
                for (int x = lo + j; x < lo + S; x += GROUP) sum += term(lf, cA, cB, M, x, cut);
            }
#pragma unroll
            for (int d = GROUP / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, GROUP);
            if (have && j == 0) {
                double pv;
                if (S > SMALL_S) {
                    pv = w.p[idx];                                    // fisher_kernel<true> has been there
                } else {
                    pv = S == 1 ? 1.0 : capped(sum);
                    w.p[idx] = pv;
                }
                atomicAdd(&lds_hist[bin_of(pv)], 1u);
                passed += pv <= alpha ? 1 : 0;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) passed += __shfl_down(passed, d, 64);
        if (lane == 0) wave_pass[wave] = passed;
        __syncthreads();
        if (threadIdx.x == 0) {
            int all = 0;
#pragma unroll
            for (int k = 0; k < THREADS / 64; ++k) all += wave_pass[k];
            chunk_n[blockIdx.x] = all;
        }
        if (threadIdx.x < HIST_BINS) {
            const unsigned v = lds_hist[threadIdx.x];
            if (v) atomicAdd(&hist[threadIdx.x], (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(THREADS) void records_kernel(const WorkList w, const double alpha, const long long* __restrict__ chunk_off, const Records r) {
    __shared__ long long wave_total[THREADS / 64];
    const long long idx = (long long)blockIdx.x * CHUNK + threadIdx.x;
    const bool listed = idx < w.n && w.p[idx] <= alpha;
    long long total;
    const long long at = chunk_off[blockIdx.x] + csites::block_exclusive_scan<THREADS>(listed ? 1 : 0, wave_total, total);
    if (listed && at < r.n) {
        const unsigned key = w.key[idx];
        r.pos[at] = int(key >> 1);
        r.strand[at] = (unsigned char)(key & 1u);
        r.cA[at] = w.cA[idx];
        r.mA[at] = w.mA[idx];
        r.cB[at] = w.cB[idx];
        r.mB[at] = w.mB[idx];
        r.p[at] = w.p[idx];
    }
}

}  // namespace dfk
