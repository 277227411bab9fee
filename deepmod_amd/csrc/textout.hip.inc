// textout.hip.inc — the tiled text writer of every command that writes lines per position on the device (part of offline.hip): merge and bslabels.
// The sibling of textlines.hip.inc on the way out.  An emitter (textout.inc; passed to the kernels by value) gives the lines of one position; the
// text of `length` positions leaves the device in bounded runs of whole tiles:
//   length_kernel<E>    a block per tile of TILE_POS positions, POS_PER_LANE consecutive ones per lane: bytes and lines of the tile (counting sink,
//                       two block scans).  An emitter that declares CHECKED skips a position that is not ok() and counts the tile into *bad_tiles.
//   xyk::scan_in_place  the 64-bit scans over the tiles: the first byte of every tile, the bytes and the lines of the text behind them
//   write_kernel<E>     the same routine with a writing sink at tile offset + block scan of the lanes' bytes
// No atomics in the text: a line's offset is a function of the emitter's tables alone and every output byte has one writer, so two runs give
// identical bytes.  Run is the state of one format between begin and the last next; its owner's entry points check their own preconditions
// in front of it and name themselves in `who`.
#pragma once
#include "host.h"
#include "blockscan.hip.inc"
#include "xyrows.hip.inc"
#include "textout.inc"

namespace txo {

constexpr int TILE_POS = 1024;                      // positions of one tile (dm_bedmerge_tile_positions, dm_bslabels_tile_positions)
constexpr int THREADS = 256;
constexpr int POS_PER_LANE = TILE_POS / THREADS;

template <class E>
__global__ __launch_bounds__(THREADS) void length_kernel(const E em, const long long length, long long* __restrict__ tile_bytes, long long* __restrict__ tile_lines) {
    __shared__ long long wave_total[THREADS / 64];
    const long long q0 = (long long)blockIdx.x * TILE_POS + (long long)threadIdx.x * POS_PER_LANE;
    CountSink c;
    int lines = 0, bad = 0;
    for (int k = 0; k < POS_PER_LANE; ++k) {
        const long long q = q0 + k;
        if (q >= length) break;
        if constexpr (E::CHECKED) {
            if (!em.ok(q)) {
                bad = 1;
                continue;
            }
        }
        lines += em(c, q, q);
    }
    long long total_bytes, total_lines;
    (void)csites::block_exclusive_scan<THREADS>(c.n, wave_total, total_bytes);
    (void)csites::block_exclusive_scan<THREADS>((long long)lines, wave_total, total_lines);
    if constexpr (E::CHECKED) bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        tile_bytes[blockIdx.x] = total_bytes;
        tile_lines[blockIdx.x] = total_lines;
        if constexpr (E::CHECKED) {
            if (bad) atomicAdd(em.bad_tiles, 1ull);
        }
    }
}

// tiles first_tile .. of the grid: their text at out + (tile_off[tile] - tile_off[first_tile])
template <class E>
__global__ __launch_bounds__(THREADS) void write_kernel(const E em, const long long length, const long long* __restrict__ tile_off, const long long first_tile,
                                                       char* __restrict__ out) {
    __shared__ long long wave_total[THREADS / 64];
    const long long tile = first_tile + blockIdx.x;
    const long long q0 = tile * TILE_POS + (long long)threadIdx.x * POS_PER_LANE;
    CountSink c;
    for (int k = 0; k < POS_PER_LANE; ++k)
        if (q0 + k < length) em(c, q0 + k, q0 + k);
    long long total;
    const long long ex = csites::block_exclusive_scan<THREADS>(c.n, wave_total, total);
    if (c.n == 0 || ex + c.n > tile_off[tile + 1] - tile_off[tile]) return;      // (never past the counted length, whatever became of the tables since)
    WriteSink w{out + (tile_off[tile] - tile_off[first_tile]) + ex};
    for (int k = 0; k < POS_PER_LANE; ++k)
        if (q0 + k < length) em(w, q0 + k, q0 + k);
}

struct Totals {
    long long lines = 0, bytes = 0, largest_tile = 0;
    unsigned long long bad_tiles = 0;               // of a CHECKED emitter (which zeroes its counter before begin)
};

struct Run {
    hipEvent_t ev[2] = {nullptr, nullptr};
    enum { TBYTES, TLINES, TEXT };
    DevBufs<3> b{nullptr};
    std::vector<long long> tile_off;                    // [tiles + 1]: the first text byte of every tile (empty: no format begun)
    int64_t next_tile = 0;
    double ms = 0.0;                                    // of the kernels so far (HIP events), for the owner's dm_*_times

    bool init(const char* handle_name) {                // the owner's name, for the message of a failed allocation
        b.who = handle_name;
        return hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    }
    void release() {
        b.release();
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }
    void clear() { tile_off.clear(); }
    bool begun() const { return !tile_off.empty(); }

    // the tiles of `length` positions counted and scanned on xy's stream -> t, behind one stream synchronisation
    template <class E>
    int begin(dm_xyrows* xy, const E& em, const int64_t length, const char* who, Totals& t) {
        clear();
        t = Totals{};
        HIP_TRY(hipSetDevice(xy->device));
        const int64_t tiles = (length + TILE_POS - 1) / TILE_POS;
        int rc;
        if ((rc = b.ensure(TBYTES, size_t(tiles + 1) * 8)) != DM_OK || (rc = b.ensure(TLINES, size_t(tiles + 1) * 8)) != DM_OK) return rc;
        hipStream_t s = xy->stream;
        long long* d_bytes = b.ptr<long long>(TBYTES);
        long long* d_lines = b.ptr<long long>(TLINES);
        HIP_TRY(hipEventRecord(ev[0], s));
        hipLaunchKernelGGL(length_kernel<E>, dim3(unsigned(tiles)), dim3(THREADS), 0, s, em, (long long)length, d_bytes, d_lines);
        HIP_TRY(hipGetLastError());
        if ((rc = xyk::scan_in_place(xy, d_bytes, tiles)) != DM_OK || (rc = xyk::scan_in_place(xy, d_lines, tiles)) != DM_OK) return rc;
        HIP_TRY(hipEventRecord(ev[1], s));
        std::vector<long long> off(size_t(tiles) + 1);
        HIP_TRY(hipMemcpyAsync(off.data(), d_bytes, off.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&t.lines, d_lines + tiles, 8, hipMemcpyDeviceToHost, s));
        if constexpr (E::CHECKED) HIP_TRY(hipMemcpyAsync(&t.bad_tiles, em.bad_tiles, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        double counting_ms = 0.0;
        if ((rc = add_time(ev[0], ev[1], counting_ms)) != DM_OK) return rc;
        if (off[0] != 0) return fail(DM_ESTATE, "%s: the first tile starts at byte %lld", who, off[0]);
        for (int64_t i = 0; i < tiles; ++i) {
            if (off[i + 1] < off[i]) return fail(DM_ESTATE, "%s: descending tile offsets", who);
            t.largest_tile = std::max(t.largest_tile, off[i + 1] - off[i]);
        }
        t.bytes = off[size_t(tiles)];
        if (t.bytes > 0) ms += counting_ms;                              // ms is the time of the texts written: tables without a line add nothing
        tile_off.swap(off);
        next_tile = 0;
        return DM_OK;
    }

    // The next run of whole tiles that fits `cap` bytes -> out, *got bytes.  em and length are those of begin (built anew: a pointer may have moved).
    // -> 1: text was returned and more follows, 0: this was the last run (or there is no text), < 0: an error
    template <class E>
    int next(dm_xyrows* xy, const E& em, const int64_t length, const char* who, char* out, const int64_t cap, int64_t* got) {
        if (cap < 0 || (cap > 0 && !out) || !got) return fail(DM_EINVAL, "%s: null argument", who);
        *got = 0;                                                        // (an error returns no text)
        const int64_t tiles = int64_t(tile_off.size()) - 1;
        const std::vector<long long>& off = tile_off;
        int64_t t0 = next_tile;
        while (t0 < tiles && off[size_t(t0) + 1] == off[size_t(t0)]) ++t0;                     // tiles without text
        if (t0 >= tiles) {
            next_tile = tiles;
            return 0;
        }
        if (off[size_t(t0) + 1] - off[size_t(t0)] > cap)
            return fail(DM_EINVAL, "%s: a buffer of %lld bytes does not hold the tile at position %lld: %lld bytes are needed", who, (long long)cap, (long long)(t0 * TILE_POS),
                        (long long)(off[size_t(t0) + 1] - off[size_t(t0)]));
        // the last tile whose end still fits: off is ascending
        const int64_t t1 = int64_t(std::upper_bound(off.begin() + t0 + 1, off.end(), off[size_t(t0)] + cap) - off.begin()) - 1;
        const int64_t bytes = off[size_t(t1)] - off[size_t(t0)];
        if (t1 <= t0 || t1 > tiles || bytes <= 0 || bytes > cap) return fail(DM_ESTATE, "%s: tiles %lld .. %lld of %lld bytes", who, (long long)t0, (long long)t1, (long long)bytes);
        HIP_TRY(hipSetDevice(xy->device));
        int rc;
        if ((rc = b.ensure(TEXT, size_t(bytes))) != DM_OK) return rc;
        hipStream_t s = xy->stream;
        HIP_TRY(hipEventRecord(ev[0], s));
        hipLaunchKernelGGL(write_kernel<E>, dim3(unsigned(t1 - t0)), dim3(THREADS), 0, s, em, (long long)length, b.ptr<const long long>(TBYTES), (long long)t0, b.ptr<char>(TEXT));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[1], s));
        HIP_TRY(hipMemcpyAsync(out, b.buf[TEXT], size_t(bytes), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if ((rc = add_time(ev[0], ev[1], ms)) != DM_OK) return rc;
        *got = bytes;
        next_tile = t1;
        while (next_tile < tiles && off[size_t(next_tile) + 1] == off[size_t(next_tile)]) ++next_tile;
        return next_tile < tiles ? 1 : 0;
    }
};

}  // namespace txo
