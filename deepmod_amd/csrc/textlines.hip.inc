// textlines.hip.inc — the line splitter of every command that parses a text on the device (part of offline.hip): predict and train --resident
// (xyparse.hip.inc), siteperf, merge and bsperf.  The bytes of a text -> the first byte of every line; the caller's own kernel then reads one
// line per lane and leaves a status byte per line, of which first_bad finds the first that is set.
// Plain launches on the stream of the handle's scan, no atomics, one writer per output element: two calls on the same bytes give the same bytes.
//   xl_count_kernel   a tile of TILE bytes, 16 per lane (one dwordx4 load): newlines counted with one ballot per byte column -> count per tile
//   xyk::scan_in_place  exclusive 64-bit scan of the tile counts: the first line of every tile, the row count R behind them
//   xl_lines_kernel   the same loads again: a newline's rank = the tile's first line + the block scan of the lane counts -> the first byte of
//                     every line
//   xl_first_kernel   one block: the smallest row with a status byte set (-1: none)
// The handle keeps the splitter's five blocks at the head of its DevBufs (TEXT .. OUT below) and numbers its own behind N_SPLIT.
#pragma once
#include "host.h"
#include "blockscan.hip.inc"
#include "xyrows.hip.inc"

namespace xlk {

constexpr int THREADS = 256;
constexpr int LANE_BYTES = 16;
constexpr int TILE = THREADS * LANE_BYTES;          // dm_xyload_tile_bytes()
constexpr int64_t MAX_BYTES = int64_t(1) << 40;
enum { TEXT, COUNT, START, STATUS, OUT, N_SPLIT };  // STATUS [rows] is sized by the caller, with its records

__device__ inline uint4 load_lane(const char* __restrict__ text, const long long off, const long long n_bytes) {
    // the buffer holds whole 16-byte groups (split sizes it so); what lies behind n_bytes is masked by newline_mask
    return off < n_bytes ? *reinterpret_cast<const uint4*>(text + off) : uint4{0u, 0u, 0u, 0u};
}

// bit j: byte j of the lane's 16 is a '\n' of the text
__device__ inline unsigned newline_mask(const uint4 v, const long long off, const long long n_bytes) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < LANE_BYTES; ++j)
        if (((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == 0x0au && off + j < n_bytes) mask |= 1u << j;
    return mask;
}

__global__ __launch_bounds__(THREADS) void xl_count_kernel(const char* __restrict__ text, const long long n_bytes, long long* __restrict__ count) {
    __shared__ int wave_count[THREADS / 64];
    const long long off = (long long)blockIdx.x * TILE + (long long)threadIdx.x * LANE_BYTES;
    const unsigned mask = newline_mask(load_lane(text, off, n_bytes), off, n_bytes);
    int c = 0;
#pragma unroll
    for (int j = 0; j < LANE_BYTES; ++j) c += __popcll(__ballot((mask >> j) & 1u));
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int k = 0; k < THREADS / 64; ++k) t += wave_count[k];
        count[blockIdx.x] = t;
    }
}

// start [R + 1]: start[r] = the first byte of line r, start[R] = the byte behind the last newline
__global__ __launch_bounds__(THREADS) void xl_lines_kernel(const char* __restrict__ text, const long long n_bytes, const long long* __restrict__ tile_row,
                                                          const long long n_rows, long long* __restrict__ start) {
    __shared__ long long wave_total[THREADS / 64];
    const long long off = (long long)blockIdx.x * TILE + (long long)threadIdx.x * LANE_BYTES;
    const unsigned mask = newline_mask(load_lane(text, off, n_bytes), off, n_bytes);
    long long total;
    long long r = tile_row[blockIdx.x] + csites::block_exclusive_scan<THREADS>((long long)__popc(mask), wave_total, total);
    if (blockIdx.x == 0 && threadIdx.x == 0) start[0] = 0;
    for (int j = 0; j < LANE_BYTES; ++j)
        if ((mask >> j) & 1u) {
            ++r;                                                     // this newline ends line r - 1
            if (r <= n_rows) start[r] = off + j + 1;
        }
}

// out[0] = the smallest i with status[i] != 0, -1 if there is none
__global__ __launch_bounds__(xyk::SUM_THREADS) void xl_first_kernel(const unsigned char* __restrict__ status, const long long n, long long* __restrict__ out) {
    __shared__ long long wave_min[xyk::SUM_THREADS / 64];
    const long long none = 0x7fffffffffffffffLL;
    long long best = none;
    for (long long i = threadIdx.x; i < n; i += xyk::SUM_THREADS)
        if (status[i] && i < best) best = i;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d, 64));
    if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < xyk::SUM_THREADS / 64; ++k) best = min(best, wave_min[k]);
        out[0] = best == none ? -1 : best;
    }
}

// The text onto the device (a missing last '\n' appended) and its line starts into START, on xy's stream.  -> *rows: its lines (0: an empty text,
// nothing was done), read back behind one stream synchronisation.  `begin` is recorded behind the upload: what follows is kernels only.
// who: the entry point, noun: what it calls a line ("<who>: %lld <noun> (at most %lld)").
template <int N>
int split(dm_xyrows* xy, DevBufs<N>& b, const char* text, const int64_t n_bytes, const int64_t max_rows, const char* who, const char* noun, hipEvent_t begin,
          long long* rows_out) {
    *rows_out = 0;
    if (n_bytes < 0 || n_bytes >= MAX_BYTES || (n_bytes > 0 && !text)) return fail(DM_EINVAL, "%s: %lld bytes of text", who, (long long)n_bytes);
    if (n_bytes == 0) return DM_OK;
    const bool add_newline = text[n_bytes - 1] != '\n';
    const int64_t n = n_bytes + (add_newline ? 1 : 0);
    const int64_t tiles = (n + TILE - 1) / TILE;
    int rc;
    if ((rc = b.ensure(TEXT, size_t(tiles) * TILE)) != DM_OK) return rc;                  // whole 16-byte groups behind every lane offset below n
    if ((rc = b.ensure(COUNT, size_t(tiles + 1) * 8)) != DM_OK) return rc;
    hipStream_t s = xy->stream;
    char* d_text = b.template ptr<char>(TEXT);
    long long* d_count = b.template ptr<long long>(COUNT);
    static const char newline = '\n';
    HIP_TRY(hipMemcpyAsync(d_text, text, size_t(n_bytes), hipMemcpyHostToDevice, s));
    if (add_newline) HIP_TRY(hipMemcpyAsync(d_text + n_bytes, &newline, 1, hipMemcpyHostToDevice, s));
    const dim3 tile_grid{unsigned(tiles)}, block{THREADS};
    HIP_TRY(hipEventRecord(begin, s));
    hipLaunchKernelGGL(xl_count_kernel, tile_grid, block, 0, s, d_text, (long long)n, d_count);
    HIP_TRY(hipGetLastError());
    if ((rc = xyk::scan_in_place(xy, d_count, tiles)) != DM_OK) return rc;
    long long rows = 0;
    HIP_TRY(hipMemcpyAsync(&rows, d_count + tiles, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (rows < 1 || rows > n) return fail(DM_ESTATE, "%s: %lld lines in %lld bytes", who, rows, (long long)n);
    if (rows > max_rows) return fail(DM_EINVAL, "%s: %lld %s (at most %lld)", who, rows, noun, (long long)max_rows);
    if ((rc = b.ensure(START, size_t(rows + 1) * 8)) != DM_OK) return rc;
    hipLaunchKernelGGL(xl_lines_kernel, tile_grid, block, 0, s, d_text, (long long)n, d_count, rows, b.template ptr<long long>(START));
    HIP_TRY(hipGetLastError());
    *rows_out = rows;
    return DM_OK;
}

// OUT[0] = the first of the `rows` bytes of STATUS that is set (-1: none): queued behind the kernel that writes them; the caller copies it back
template <int N>
int first_bad(dm_xyrows* xy, DevBufs<N>& b, const long long rows) {
    const int rc = b.ensure(OUT, 16);
    if (rc) return rc;
    hipLaunchKernelGGL(xl_first_kernel, dim3(1), dim3(xyk::SUM_THREADS), 0, xy->stream, b.template ptr<const unsigned char>(STATUS), rows, b.template ptr<long long>(OUT));
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

}  // namespace xlk
