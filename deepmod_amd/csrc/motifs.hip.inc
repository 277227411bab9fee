// motifs.hip.inc — `motifs`, the kernel (part of offline.hip through motifs.inc, which states the rule of a key and holds the handle): one sweep
// over a contig joins the sample's and the controls' counters (dm_summary tables: touch | cov | mod, `length` ints each) with the contig's bytes and
// counts per oriented sequence context how many keys were tested and how many were called modified.
//   mo_count_kernel<LDS_HIST>   a workgroup takes tiles of mok::TILE_POS positions (grid-stride over the tiles, at most MAX_BLOCKS workgroups):
//       stage      the tile's bytes plus a halo of 8 on each side -> one code byte each in LDS (2-bit code, bit 2: outside the contig or no A, C, G, T)
//       join       lane i reads position tile + i + 256 k of the 4 or 8 table columns: every load of a wave is one run of 256 bytes
//       decide     mok::fate per strand from the LDS codes: the routine dm_motifs_count_host runs; the percentage rules in 64-bit products
//       count      LDS_HIST (U + D <= mok::LDS_FLANK): 32-bit atomics into the workgroup's LDS copy of the two-column histogram, whose non-zero
//                  bins are flushed once, at the end, with 64-bit global atomics.  Otherwise 64-bit global atomics per key, after the lanes of a wave
//                  that hold the same bin at consecutive positions (a low-complexity stretch) have been merged into one add, as summary_add_kernel
//                  merges runs of one position
//       counters   five per strand and off_base in registers, reduced per wave by shuffles, across the waves in LDS: one 64-bit atomic per
//                  workgroup and counter that has something to add
// Counter widths.  A workgroup sweeps at most ceil(2^21 / MAX_BLOCKS) = 1024 tiles of 2048 keys, so a lane's 32-bit registers and a 32-bit LDS bin
// stay below 2^22; everything in global memory is 64-bit.  No counter can wrap on a contig of 2 (2^31 - 1) keys, nor over 2^31 such contigs.
// Exactness and determinism: every value is an integer sum; additions commute, so the order the atomics land in does not matter.
// Bounds: a code index is position - tile + 8 + j with |j| <= 8, inside [0, TILE_POS + 16); a table index is < length; a bin is < 4^(U+D) because
// every digit of a context without a BAD byte is 0..3.
#pragma once
#include "host.h"
#define DM_MOTIFS_RULE_ONLY
#include "motifs.inc"
#undef DM_MOTIFS_RULE_ONLY

namespace mok {

constexpr int THREADS = 256;
constexpr int HALO = MAX_FLANK;
constexpr int MAX_BLOCKS = 2048;
constexpr int PER_LANE = TILE_POS / THREADS;      // positions of a tile per lane, THREADS apart
constexpr int N_SWEEP = 2 * N_COUNT + 2;            // the sweep's counters: [2 strands][N_COUNT], off_base [2]
constexpr int LDS_BINS = 1 << (2 * LDS_FLANK);

struct TileCodes {
    const unsigned char* code;                      // LDS: code[q - first] of positions first .. first + TILE_POS + 2 HALO - 1
    long long first;
    __host__ __device__ unsigned operator()(const long long q) const { return code[q - first]; }
};

template <bool LDS_HIST>
__global__ __launch_bounds__(THREADS) void mo_count_kernel(const unsigned char* __restrict__ seq, const long long length, const int* __restrict__ plus,
                                                          const int* __restrict__ minus, const int* __restrict__ ctrl_plus, const int* __restrict__ ctrl_minus, const Rule r,
                                                          unsigned long long* __restrict__ hist, unsigned long long* __restrict__ counts) {
    __shared__ unsigned char code[TILE_POS + 2 * HALO];
    __shared__ unsigned lds_hist[LDS_HIST ? 2 * LDS_BINS : 2];
    __shared__ long long part[THREADS / 64][N_SWEEP];
    const int bins2 = 2 << (2 * (r.up + r.down));
    const int lane = threadIdx.x & 63;
    const bool ctrl = ctrl_plus != nullptr;
    if (LDS_HIST) {
        for (int i = threadIdx.x; i < bins2; i += THREADS) lds_hist[i] = 0u;
    }
    unsigned n[N_SWEEP];
#pragma unroll
    for (int k = 0; k < N_SWEEP; ++k) n[k] = 0u;
    const long long tiles = (length + TILE_POS - 1) / TILE_POS;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long q0 = tile * TILE_POS;
        __syncthreads();                                              // the codes of the tile before are no longer read (and lds_hist is zeroed)
        for (int i = threadIdx.x; i < TILE_POS + 2 * HALO; i += THREADS) {
            const long long q = q0 - HALO + i;
            code[i] = (unsigned char)(q < 0 || q >= length ? BAD : code_of(seq[q]));
        }
        __syncthreads();
        const TileCodes at = {code, q0 - HALO};
        for (int k = 0; k < PER_LANE; ++k) {                          // whole waves iterate together: the ballots below see all 64 lanes
            const long long p = q0 + (long long)k * THREADS + threadIdx.x;
            const bool in = p < length;
            int cv[2] = {0, 0}, md[2] = {0, 0}, ccv[2] = {0, 0}, cmd[2] = {0, 0};
            if (in) {
                cv[0] = plus[length + p];
                md[0] = plus[2 * length + p];
                cv[1] = minus[length + p];
                md[1] = minus[2 * length + p];
                if (ctrl) {
                    ccv[0] = ctrl_plus[length + p];
                    cmd[0] = ctrl_plus[2 * length + p];
                    ccv[1] = ctrl_minus[length + p];
                    cmd[1] = ctrl_minus[2 * length + p];
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                unsigned ctx = 0;
                const int f = in ? fate(at, p, s, r, cv[s], md[s], ctrl, ccv[s], cmd[s], ctx) : int(F_IGNORED);
                const bool tested = f == F_TESTED || f == F_MODIFIED, modified = f == F_MODIFIED;
#pragma unroll
                for (int j = 0; j < N_COUNT; ++j) n[s * N_COUNT + j] += (f == j || (j == K_TESTED && modified)) ? 1u : 0u;
                n[2 * N_COUNT + s] += f == F_OFF_BASE ? 1u : 0u;
                if (LDS_HIST) {
                    if (tested) atomicAdd(&lds_hist[2 * ctx], 1u);
                    if (modified) atomicAdd(&lds_hist[2 * ctx + 1], 1u);
                } else {
                    // lanes are consecutive positions: a run of lanes with one bin becomes one add of its head
                    const long long key = tested ? (long long)ctx : -1 - lane;        // a lane without a bin: a key of its own, never merged
                    const long long before = __shfl_up(key, 1, 64);
                    const bool head = lane == 0 || key != before;
                    const unsigned long long heads = __ballot(head), m_mod = __ballot(modified);
                    if (head && tested) {
                        const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
                        const int len = above ? __ffsll((long long)above) : 64 - lane;                   // the run is [lane, next head)
                        const unsigned long long run = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
                        atomicAdd(&hist[2 * (unsigned long long)ctx], (unsigned long long)len);
                        const int nm = __popcll(m_mod & run);
                        if (nm) atomicAdd(&hist[2 * (unsigned long long)ctx + 1], (unsigned long long)nm);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (LDS_HIST) {
        for (int i = threadIdx.x; i < bins2; i += THREADS) {
            const unsigned v = lds_hist[i];
            if (v) atomicAdd(&hist[i], (unsigned long long)v);
        }
    }
#pragma unroll
    for (int k = 0; k < N_SWEEP; ++k) {
        long long v = n[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) part[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < N_SWEEP) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) v += part[w][threadIdx.x];
        if (v != 0) atomicAdd(counts + threadIdx.x, (unsigned long long)v);
    }
}

}  // namespace mok
