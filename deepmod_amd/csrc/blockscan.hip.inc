// blockscan.hip.inc — the block-wide scan that the site stage (cluster_sites.hip.inc), getfeatures (xyrows.hip.inc) and the .xy parser
// (xyparse.hip.inc) share.  A device header: two translation units include it, so everything in it is inline.
#pragma once
#include <hip/hip_runtime.h>

namespace csites {

// exclusive scan of one value per thread over the block; total = the block's sum.  Every thread of the block calls it.
template <int NT>
__device__ inline long long block_exclusive_scan(const long long v, long long* wave_total /* LDS [NT / 64] */, long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wave_total[w] = inc;
    __syncthreads();
    long long before = 0;
    total = 0;
    for (int k = 0; k < NT / 64; ++k) {
        const long long t = wave_total[k];
        if (k < w) before += t;
        total += t;
    }
    __syncthreads();                                          // wave_total may be written again
    return before + inc - v;
}

}  // namespace csites
