// diffrep.hip.inc — `diffmod --replicates 1`, the kernel (part of offline.hip through diffrep.inc, which states the fate of a key and the
// quasi-binomial F test and holds the handle).  One run joins the tables of n_a sample and n_b control replicates (dm_summary tables: touch | cov | mod,
// `length` ints each) and tests every key with enough deep replicates in both groups.
//   sweep_kernel<WRITE>   a workgroup takes tiles of dfk::TILE_POS positions (grid-stride over the tiles, at most MAX_BLOCKS workgroups); lane i reads
//                         position tile + i + 256 k of the cov / mod columns of every replicate and strand (every load of a wave is one run of 256
//                         bytes; the table pointers come by value in one struct) and runs dfr::test_key, O(replicates) work per key, so there is
//                         no work list.  Launched twice: <false> counts - the four counters of either strand (registers, shuffles, LDS, one 64-bit
//                         atomic per workgroup and counter), the p histogram of every tested key (32-bit LDS atomics, flushed with 64-bit global
//                         ones) and the keys with p <= alpha of every tile; <true>, after dfk::scan_kernel has turned those into offsets, tests
//                         the keys again and writes the records in key order (ascending position, '+' before '-'; a block scan per slab of 256
//                         positions).
// Determinism: a key's p is a function of its counts alone (no reduction across lanes enters it), so the two launches and two runs give the same bits.
// Bounds: a table index is < length; a record index is < n_records by the scan, and checked again at every store; a histogram bin is < 20 by
// dfk::bin_of.  Only vector stores and atomics; no inline assembly.
#pragma once
#include "host.h"
#include "blockscan.hip.inc"
#include "diffmod.hip.inc"
#define DM_DIFFREP_RULE_ONLY
#include "diffrep.inc"
#undef DM_DIFFREP_RULE_ONLY

namespace dfr {

constexpr int THREADS = dfk::THREADS;
constexpr int TILE_POS = dfk::TILE_POS;             // positions of one tile of the sweep (dm_diffmod_tile_positions)
constexpr int PER_LANE = TILE_POS / THREADS;        // positions of a tile per lane, THREADS apart
constexpr int MAX_BLOCKS = 2048;
enum { W_RECORDS = 2 * N_COUNT, N_WORDS };          // the 64-bit words of a run: the counters [2][N_COUNT], then the number of records

struct Tables {
    const int* t[2][SLOTS];                         // [strand][slot]: the table of the slot's replicate, null for a slot without one
};

struct Records {
    int* pos;
    unsigned char* strand;
    int *cA, *mA, *cB, *mB;
    unsigned char *nA, *nB;
    double *phi, *p;
    long long n;
};

template <bool WRITE>
__global__ __launch_bounds__(THREADS) void sweep_kernel(const long long length, const Tables tab, const Rule rule, int* __restrict__ tile_n,
                                                       const long long* __restrict__ tile_off, const Records r, unsigned long long* __restrict__ counts,
                                                       unsigned long long* __restrict__ hist) {
    __shared__ long long wave_total[THREADS / 64];
    __shared__ long long part[THREADS / 64][2 * N_COUNT];
    __shared__ unsigned lds_hist[HIST_BINS];
    const int lane = threadIdx.x & 63;
    unsigned n[2 * N_COUNT];
#pragma unroll
    for (int k = 0; k < 2 * N_COUNT; ++k) n[k] = 0u;
    if (!WRITE) {
        if (threadIdx.x < HIST_BINS) lds_hist[threadIdx.x] = 0u;
        __syncthreads();
    }
    const long long tiles = (length + TILE_POS - 1) / TILE_POS;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long q0 = tile * TILE_POS;
        long long base = WRITE ? tile_off[tile] : 0;
        for (int k = 0; k < PER_LANE; ++k) {                          // the whole workgroup iterates together: block_exclusive_scan has barriers
            const long long p = q0 + (long long)k * THREADS + threadIdx.x;
            const bool in = p < length;
            Tested t[2];
            bool listed[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                int c[SLOTS], m[SLOTS];
#pragma unroll
                for (int i = 0; i < SLOTS; ++i) {
                    const int* const table = tab.t[s][i];
                    c[i] = m[i] = 0;
                    if (table != nullptr && in) {
                        c[i] = table[length + p];
                        m[i] = table[2 * length + p];
                    }
                }
                const int f = in ? test_key(rule, c, m, t[s]) : int(F_IGNORED);
                listed[s] = f == F_TESTED && t[s].p <= rule.alpha;
                if (!WRITE) {
#pragma unroll
                    for (int j = 0; j < N_COUNT; ++j) n[s * N_COUNT + j] += f == j ? 1u : 0u;
                    if (f == F_TESTED) atomicAdd(&lds_hist[dfk::bin_of(t[s].p)], 1u);
                }
            }
            long long total;
            const long long before = csites::block_exclusive_scan<THREADS>((listed[0] ? 1 : 0) + (listed[1] ? 1 : 0), wave_total, total);
            if (WRITE) {
                long long at = base + before;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (!listed[s]) continue;
                    if (at < r.n) {
                        r.pos[at] = int(p);
                        r.strand[at] = (unsigned char)s;
                        r.cA[at] = t[s].cA;
                        r.mA[at] = t[s].mA;
                        r.cB[at] = t[s].cB;
                        r.mB[at] = t[s].mB;
                        r.nA[at] = (unsigned char)t[s].nA;
                        r.nB[at] = (unsigned char)t[s].nB;
                        r.phi[at] = t[s].phi;
                        r.p[at] = t[s].p;
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
    __syncthreads();                                                  // and every LDS atomic of the histogram has landed
    if (threadIdx.x < 2 * N_COUNT) {
        long long v = 0;
#pragma unroll
        for (int wv = 0; wv < THREADS / 64; ++wv) v += part[wv][threadIdx.x];
        if (v != 0) atomicAdd(counts + threadIdx.x, (unsigned long long)v);
    }
    if (threadIdx.x < HIST_BINS) {
        const unsigned v = lds_hist[threadIdx.x];
        if (v) atomicAdd(&hist[threadIdx.x], (unsigned long long)v);
    }
}

}  // namespace dfr
