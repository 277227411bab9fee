// xyrows.hip.inc — getfeatures, device part (part of offline.hip): which matrix rows of a batch are kept, and their text.
//
// Replaces myGetFeatureBasedPos.py:512-526 (a row is kept if a labelled row of its read lies within +-25 rows; more than 0.9 of the rows kept: all of
// them; none: the read gives nothing) and np.savetxt(fmt='%.3f') of the kept rows (:123, :343), for all reads of a batch at once and without the
// [R][10] matrix: a row is (pos, lab, code) from the host walk (xyrows.inc) + the (mean, stdv, length) of its event in the block the signal stage left
// on the device.  Byte kernels, HBM-bound, plain launches on one stream:
//   xy_dilate_kernel   a 256-row tile: the labelled rows of the tile and of 64 rows on either side as six ballot words in LDS; a row's window, cut
//                      to its read, is a mask over at most two of them.  -> one 0 / 1 per row
//   scan (three kernels)  exclusive 64-bit scan of an array in place, the total behind it
//   xy_rule_kernel     per read: kept = the difference of the scan at its ends -> 0 nothing | 1 the dilated rows | 2 all rows, and its row count
//   xy_length_kernel   per row: kept or not, and the bytes of its text (emit_row with a counting sink); a value the formatter does not take raises the
//                      block's flag word
//   xy_finish_kernel   per read its first text byte; the flag words ORed into one
//   xy_write_kernel    per kept row: emit_row with a writing sink at the row's scanned offset
// No atomics: every output byte has one writer (the flag is a per-block word, then one OR by one block), so two runs give identical bytes.
// Formatting (checked against Python's '%.3f' on random fp32 patterns below 2^30 and on every k / 2000 with its fp32 neighbours): the sign is the sign
// bit; q = rint(double(|v|) * 1000.0) - the product of an fp32 and 1000 is exact in double, rint rounds the tie to even as the correctly rounded decimal
// does; the digits are q / 1000 '.' q % 1000 on three places.
#pragma once
#include "host.h"
#include "blockscan.hip.inc"
#include "textout.inc"
#include "xyrows.inc"

struct dm_xyrows {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    enum { POS, LAB, CODE, RDESC, SCAN, LEN, KEEP, BSUM, RCOUNT, RMODE, RBYTE, BFLAG, OUT, TEXT, N_BUF };
    DevBufs<N_BUF> b{"dm_xy_rows"};
    int64_t n_reads = 0, n_rows = 0, n_bytes = -1;      // of the last call (n_bytes < 0: none)
    bool host_result = false, timed = false;            // the last call went through dm_xy_rows_host: its results are the vectors below
    std::vector<char> h_text;
    std::vector<uint8_t> h_keep;
    std::vector<int64_t> h_row_off, h_byte_off;
};

namespace xyk {

constexpr int THREADS = 256;
constexpr int NB = 25;                  // :516
constexpr int SCAN_PER_THREAD = 4;
constexpr int SCAN_TILE = THREADS * SCAN_PER_THREAD;
constexpr int SUM_THREADS = 1024;

// the last read whose first row is <= q
__device__ inline int read_of_row(const long long* __restrict__ rdesc, const int n_reads, const long long q) {
    int lo = 0, hi = n_reads - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rdesc[4 * (long long)mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(THREADS) void xy_dilate_kernel(const unsigned char* __restrict__ lab, const long long* __restrict__ rdesc, const int n_reads,
                                                           const long long n_rows, long long* __restrict__ dil /* [n_rows] */) {
    __shared__ unsigned long long word[6];                           // rows base - 64 .. base + 319, bit = row is labelled
    const long long base = (long long)blockIdx.x * THREADS;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long q = base + threadIdx.x;
    const unsigned long long own = __ballot(q < n_rows && lab[q] != 0);
    if (lane == 0) word[1 + w] = own;
    if (w < 2) {                                                     // wave 0: the 64 rows before the tile, wave 1: the 64 rows behind it
        const long long h = w == 0 ? base - 64 + lane : base + THREADS + lane;
        const unsigned long long halo = __ballot(h >= 0 && h < n_rows && lab[h] != 0);
        if (lane == 0) word[w == 0 ? 0 : 5] = halo;
    }
    __syncthreads();
    if (q >= n_rows) return;
    const int r = read_of_row(rdesc, n_reads, q);
    const long long r0 = rdesc[4 * (long long)r], r1 = r + 1 < n_reads ? rdesc[4 * (long long)(r + 1)] : n_rows;
    const long long lo = max(q - NB, r0), hi = min(q + NB, r1 - 1);  // r0 <= q < r1: lo <= q <= hi, both within 25 rows of the tile
    const int bl = int(lo - (base - 64)), bh = int(hi - (base - 64));
    const unsigned long long from = ~0ull << (bl & 63), upto = ~0ull >> (63 - (bh & 63));
    const unsigned long long hit = (bl >> 6) == (bh >> 6) ? (word[bl >> 6] & from & upto) : ((word[bl >> 6] & from) | (word[bh >> 6] & upto));
    dil[q] = hit ? 1 : 0;
}

// ---- exclusive scan of a[0 .. n) in place, a[n] = the total: tiles, their sums by one block, the sums added back ----
__global__ __launch_bounds__(THREADS) void scan_tile_kernel(long long* __restrict__ a, const long long n, long long* __restrict__ bsum) {
    __shared__ long long wave_total[THREADS / 64];
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_PER_THREAD;
    long long v[SCAN_PER_THREAD], mine = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        v[k] = i0 + k < n ? a[i0 + k] : 0;
        mine += v[k];
    }
    long long total;
    long long ex = csites::block_exclusive_scan<THREADS>(mine, wave_total, total);
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        if (i0 + k < n) a[i0 + k] = ex;
        ex += v[k];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(SUM_THREADS) void scan_sums_kernel(long long* __restrict__ bsum, const long long m) {       // in place, bsum[m] = the total
    __shared__ long long wave_total[SUM_THREADS / 64];
    long long carry = 0;
    for (long long base = 0; base < m; base += SUM_THREADS) {
        const long long i = base + threadIdx.x;
        long long total;
        const long long ex = csites::block_exclusive_scan<SUM_THREADS>(i < m ? bsum[i] : 0, wave_total, total);
        if (i < m) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[m] = carry;
}

__global__ __launch_bounds__(THREADS) void scan_add_kernel(long long* __restrict__ a, const long long n, const long long* __restrict__ bsum, const long long m) {
    const long long add = bsum[blockIdx.x];
    const long long i0 = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_PER_THREAD;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
        if (i0 + k < n) a[i0 + k] += add;
    if (blockIdx.x == 0 && threadIdx.x == 0) a[n] = bsum[m];
}

// per read: 0 nothing | 1 the dilated rows | 2 the whole matrix, and the rows it gives (10 kept > 9 n is len(keepInd) > len(mfeatures) * 0.9: the double
// product n * 0.9 is the exact integer for every multiple of ten up to 4e7, and a comparison of an integer with a non-integer product agrees as well)
__global__ __launch_bounds__(THREADS) void xy_rule_kernel(const long long* __restrict__ scan, const long long* __restrict__ rdesc, const int n_reads,
                                                         const long long n_rows, unsigned char* __restrict__ rmode, long long* __restrict__ rcount) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_reads) return;
    const long long r0 = rdesc[4 * (long long)r], r1 = r + 1 < n_reads ? rdesc[4 * (long long)(r + 1)] : n_rows;
    const long long kept = scan[r1] - scan[r0], n = r1 - r0;
    const int mode = kept == 0 ? 0 : (10 * kept > 9 * n ? 2 : 1);
    rmode[r] = (unsigned char)mode;
    rcount[r] = mode == 2 ? n : kept;
}

using txo::CountSink;                                                // the sinks and the digits of every text writer (textout.inc)
using txo::WriteSink;
using txo::put_uint;

template <class Sink>
__device__ inline void put_flag(Sink& s, const bool one) {           // 0.000 / 1.000 and the space behind it
    s.put(one ? '1' : '0');
    s.put('.');
    s.put('0');
    s.put('0');
    s.put('0');
    s.put(' ');
}

// what the formatter takes: finite and below 2^30 in magnitude (q < 2^40; the integer part fits 32 bits)
__device__ inline bool value_ok(const float v) { return fabsf(v) < 1073741824.0f; }

template <class Sink>
__device__ inline void put_value(Sink& s, const float v, const char end) {
    if (__float_as_uint(v) >> 31) s.put('-');
    const unsigned long long q = (unsigned long long)rint(double(fabsf(v)) * 1000.0);
    const unsigned ip = unsigned(q / 1000ull), fp = unsigned(q - 1000ull * ip);
    put_uint(s, ip);
    s.put('.');
    s.put(char('0' + fp / 100));
    s.put(char('0' + fp / 10 % 10));
    s.put(char('0' + fp % 10));
    s.put(end);
}

// one row of the file.  The same routine counts (xy_length_kernel) and writes (xy_write_kernel): the two cannot disagree on a length.
template <class Sink>
__device__ inline void emit_row(Sink& s, const long long pos, const unsigned lab, const unsigned code, const float mean, const float stdv, const float len) {
    put_uint(s, (unsigned long long)pos);                            // 0 <= pos < 2^53 (dm_xy_rows): '%.3f' of the double is the integer and .000
    s.put('.');
    s.put('0');
    s.put('0');
    s.put('0');
    s.put(' ');
    put_flag(s, lab == 1u);
    put_flag(s, lab == 2u);
    put_flag(s, code == 0u);
    put_flag(s, code == 1u);
    put_flag(s, code == 2u);
    put_flag(s, code == 3u);
    put_value(s, mean, ' ');
    put_value(s, stdv, ' ');
    put_value(s, len, '\n');
}

struct RowValues {
    float mean, stdv, len;
    bool ok;
};

// columns 7..9 of row q of read r (rows_assemble_kernel's rule); values the formatter does not take are replaced by 0 and reported
__device__ inline RowValues row_values(const float* __restrict__ ev3, const long long* __restrict__ d, const long long q) {
    const long long e = q + d[1];
    RowValues v{0.0f, 0.0f, 0.0f, true};
    if (e >= d[2] && e < d[3]) {
        v.mean = ev3[3 * e];
        v.stdv = ev3[3 * e + 1];
        v.len = ev3[3 * e + 2];
        v.ok = value_ok(v.mean) && value_ok(v.stdv) && v.len >= 0.0f && v.len <= 16777216.0f;
        if (!v.ok) v.mean = v.stdv = v.len = 0.0f;
    }
    return v;
}

__global__ __launch_bounds__(THREADS) void xy_length_kernel(const long long* __restrict__ pos, const unsigned char* __restrict__ lab, const unsigned char* __restrict__ code,
                                                           const float* __restrict__ ev3, const long long* __restrict__ rdesc, const int n_reads,
                                                           const long long n_rows, const long long* __restrict__ scan, const unsigned char* __restrict__ rmode,
                                                           unsigned char* __restrict__ keep, long long* __restrict__ len, unsigned* __restrict__ bflag) {
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    int bad = 0;
    if (q < n_rows) {
        const int r = read_of_row(rdesc, n_reads, q);
        const unsigned mode = rmode[r];
        const bool k = mode == 2u || (mode == 1u && scan[q + 1] != scan[q]);
        long long n = 0;
        if (k) {
            const RowValues v = row_values(ev3, rdesc + 4 * (long long)r, q);
            bad = v.ok ? 0 : 1;
            CountSink s;
            emit_row(s, pos[q], lab[q], code[q], v.mean, v.stdv, v.len);
            n = s.n;
        }
        keep[q] = k ? 1 : 0;
        len[q] = n;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) bflag[blockIdx.x] = unsigned(bad != 0);
}

// out[0] = 1 if a block raised its flag; rbyte[r] = the first text byte of read r (the scanned lengths at its first row), rbyte[n_reads] = all bytes
__global__ __launch_bounds__(THREADS) void xy_finish_kernel(const unsigned* __restrict__ bflag, const long long n_blocks, const long long* __restrict__ len_scan,
                                                           const long long* __restrict__ rdesc, const int n_reads, const long long n_rows,
                                                           long long* __restrict__ rbyte, long long* __restrict__ out) {
    int bad = 0;
    for (long long b = threadIdx.x; b < n_blocks; b += THREADS) bad |= int(bflag[b]);
    for (int r = threadIdx.x; r <= n_reads; r += THREADS) rbyte[r] = len_scan[r < n_reads ? rdesc[4 * (long long)r] : n_rows];
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) out[0] = bad != 0;
}

__global__ __launch_bounds__(THREADS) void xy_write_kernel(const long long* __restrict__ pos, const unsigned char* __restrict__ lab, const unsigned char* __restrict__ code,
                                                          const float* __restrict__ ev3, const long long* __restrict__ rdesc, const int n_reads,
                                                          const long long n_rows, const unsigned char* __restrict__ keep, const long long* __restrict__ len_scan,
                                                          char* __restrict__ text) {
    const long long q = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= n_rows || !keep[q]) return;
    const int r = read_of_row(rdesc, n_reads, q);
    const RowValues v = row_values(ev3, rdesc + 4 * (long long)r, q);
    WriteSink s{text + len_scan[q]};
    emit_row(s, pos[q], lab[q], code[q], v.mean, v.stdv, v.len);
}

// exclusive scan of n values in place (a holds n + 1), on the handle's stream
int scan_in_place(dm_xyrows* h, long long* a, int64_t n) {
    const int64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    int rc = h->b.ensure(dm_xyrows::BSUM, size_t(tiles + 1) * 8);
    if (rc) return rc;
    long long* bsum = static_cast<long long*>(h->b.buf[dm_xyrows::BSUM]);
    hipLaunchKernelGGL(scan_tile_kernel, dim3(unsigned(tiles)), dim3(THREADS), 0, h->stream, a, (long long)n, bsum);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SUM_THREADS), 0, h->stream, bsum, (long long)tiles);
    hipLaunchKernelGGL(scan_add_kernel, dim3(unsigned(tiles)), dim3(THREADS), 0, h->stream, a, (long long)n, bsum, (long long)tiles);
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

}  // namespace xyk

extern "C" {

dm_xyrows* dm_xy_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_xy_create: no device %d", device);
        return nullptr;
    }
    dm_xyrows* h = new dm_xyrows;
    h->device = device;
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < 3; ++i) ok = hipEventCreate(&h->ev[i]) == hipSuccess;
    if (!ok) {
        fail(DM_EDEVICE, "dm_xy_create: stream or events on device %d", device);
        dm_xy_destroy(h);
        return nullptr;
    }
    return h;
}

void dm_xy_destroy(dm_xyrows* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    h->b.release();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int64_t dm_xy_rows(dm_xyrows* h, const int64_t* pos, const uint8_t* lab, const uint8_t* code, const int64_t* rdesc, int64_t n_reads, int64_t n_rows,
                   const float* d_ev3, int64_t n_events, int32_t* flag) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->n_bytes = -1;
    h->timed = false;
    if (flag) *flag = 0;
    if (!pos || !lab || !code) return fail(DM_EINVAL, "dm_xy_rows: null array");
    int rc = xyhost::check_rdesc(rdesc, n_reads, n_rows, n_events, "dm_xy_rows");
    if (rc) return rc;
    if (n_events > 0 && !is_device_ptr(d_ev3)) return fail(DM_EINVAL, "dm_xy_rows: the statistics are a device block");
    for (int64_t q = 0; q < n_rows; ++q)                             // '%.3f' of the double: the device prints the integer
        if (pos[q] < 0 || pos[q] >= (int64_t(1) << 53)) return fail(DM_EINVAL, "dm_xy_rows: position %lld of row %lld", (long long)pos[q], (long long)q);
    HIP_TRY(hipSetDevice(h->device));
    using B = dm_xyrows;
    const int64_t blocks = (n_rows + xyk::THREADS - 1) / xyk::THREADS;
    const size_t need[B::N_BUF] = {size_t(n_rows) * 8, size_t(n_rows), size_t(n_rows), size_t(n_reads) * 32, size_t(n_rows + 1) * 8, size_t(n_rows + 1) * 8,
                                   size_t(n_rows), 0, size_t(n_reads + 1) * 8, size_t(n_reads), size_t(n_reads + 1) * 8, size_t(blocks) * 4, 16, 0};
    for (int i = 0; i < B::N_BUF; ++i)
        if (need[i] && (rc = h->b.ensure(i, need[i])) != DM_OK) return rc;
    long long* d_pos = static_cast<long long*>(h->b.buf[B::POS]);
    unsigned char* d_lab = static_cast<unsigned char*>(h->b.buf[B::LAB]);
    unsigned char* d_code = static_cast<unsigned char*>(h->b.buf[B::CODE]);
    long long* d_rdesc = static_cast<long long*>(h->b.buf[B::RDESC]);
    long long* d_scan = static_cast<long long*>(h->b.buf[B::SCAN]);
    long long* d_len = static_cast<long long*>(h->b.buf[B::LEN]);
    unsigned char* d_keep = static_cast<unsigned char*>(h->b.buf[B::KEEP]);
    long long* d_rcount = static_cast<long long*>(h->b.buf[B::RCOUNT]);
    unsigned char* d_rmode = static_cast<unsigned char*>(h->b.buf[B::RMODE]);
    long long* d_rbyte = static_cast<long long*>(h->b.buf[B::RBYTE]);
    unsigned* d_bflag = static_cast<unsigned*>(h->b.buf[B::BFLAG]);
    long long* d_out = static_cast<long long*>(h->b.buf[B::OUT]);
    HIP_TRY(hipMemcpyAsync(d_pos, pos, size_t(n_rows) * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_lab, lab, size_t(n_rows), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_code, code, size_t(n_rows), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_rdesc, rdesc, size_t(n_reads) * 32, hipMemcpyHostToDevice, h->stream));
    const dim3 row_grid{unsigned(blocks)}, read_grid{unsigned((n_reads + xyk::THREADS - 1) / xyk::THREADS)}, block{xyk::THREADS};
    // ---- xy_keep ----
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(xyk::xy_dilate_kernel, row_grid, block, 0, h->stream, d_lab, d_rdesc, int(n_reads), (long long)n_rows, d_scan);
    if ((rc = xyk::scan_in_place(h, d_scan, n_rows)) != DM_OK) return rc;
    hipLaunchKernelGGL(xyk::xy_rule_kernel, read_grid, block, 0, h->stream, d_scan, d_rdesc, int(n_reads), (long long)n_rows, d_rmode, d_rcount);
    if ((rc = xyk::scan_in_place(h, d_rcount, n_reads)) != DM_OK) return rc;
    HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    // ---- xy_text: lengths, their scan, the rows ----
    hipLaunchKernelGGL(xyk::xy_length_kernel, row_grid, block, 0, h->stream, d_pos, d_lab, d_code, d_ev3, d_rdesc, int(n_reads), (long long)n_rows, d_scan, d_rmode,
                       d_keep, d_len, d_bflag);
    if ((rc = xyk::scan_in_place(h, d_len, n_rows)) != DM_OK) return rc;
    hipLaunchKernelGGL(xyk::xy_finish_kernel, dim3(1), block, 0, h->stream, d_bflag, (long long)blocks, d_len, d_rdesc, int(n_reads), (long long)n_rows, d_rbyte, d_out);
    HIP_TRY(hipGetLastError());
    long long out[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&out[0], d_out, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&out[1], d_len + n_rows, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->n_reads = n_reads;
    h->n_rows = n_rows;
    h->host_result = out[0] != 0;
    if (h->host_result) {                                            // the batch holds a value the formatter does not take: the host's bytes instead
        if (flag) *flag = 1;
        std::vector<float> ev3(size_t(n_events) * 3);
        HIP_TRY(hipMemcpy(ev3.data(), d_ev3, ev3.size() * 4, hipMemcpyDeviceToHost));
        h->h_keep.resize(size_t(n_rows));
        h->h_row_off.resize(size_t(n_reads) + 1);
        h->h_byte_off.resize(size_t(n_reads) + 1);
        const int64_t total = dm_xy_rows_host(pos, lab, code, rdesc, n_reads, n_rows, ev3.data(), n_events, h->h_keep.data(), h->h_row_off.data(),
                                              h->h_byte_off.data(), nullptr, 0);
        if (total < 0) return total;
        h->h_text.resize(size_t(total));
        if (dm_xy_rows_host(pos, lab, code, rdesc, n_reads, n_rows, ev3.data(), n_events, nullptr, nullptr, nullptr, h->h_text.data(), total) != total)
            return fail(DM_ESTATE, "dm_xy_rows: the host formatter disagrees with itself");
        h->n_bytes = total;
        return total;
    }
    const int64_t total = out[1];
    if (total > 0) {
        if ((rc = h->b.ensure(B::TEXT, size_t(total))) != DM_OK) return rc;
        hipLaunchKernelGGL(xyk::xy_write_kernel, row_grid, block, 0, h->stream, d_pos, d_lab, d_code, d_ev3, d_rdesc, int(n_reads), (long long)n_rows, d_keep, d_len,
                           static_cast<char*>(h->b.buf[B::TEXT]));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->timed = true;
    h->n_bytes = total;
    return total;
}

int dm_xy_rows_fetch(dm_xyrows* h, char* text, uint8_t* keep, int64_t* read_row_off, int64_t* read_byte_off) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (h->n_bytes < 0) return fail(DM_ESTATE, "dm_xy_rows_fetch: no batch");
    if (h->host_result) {
        if (text) std::memcpy(text, h->h_text.data(), h->h_text.size());
        if (keep) std::memcpy(keep, h->h_keep.data(), h->h_keep.size());
        if (read_row_off) std::memcpy(read_row_off, h->h_row_off.data(), h->h_row_off.size() * 8);
        if (read_byte_off) std::memcpy(read_byte_off, h->h_byte_off.data(), h->h_byte_off.size() * 8);
        return DM_OK;
    }
    using B = dm_xyrows;
    HIP_TRY(hipSetDevice(h->device));
    if (text && h->n_bytes > 0) HIP_TRY(hipMemcpyAsync(text, h->b.buf[B::TEXT], size_t(h->n_bytes), hipMemcpyDeviceToHost, h->stream));
    if (keep) HIP_TRY(hipMemcpyAsync(keep, h->b.buf[B::KEEP], size_t(h->n_rows), hipMemcpyDeviceToHost, h->stream));
    if (read_row_off) HIP_TRY(hipMemcpyAsync(read_row_off, h->b.buf[B::RCOUNT], size_t(h->n_reads + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    if (read_byte_off) HIP_TRY(hipMemcpyAsync(read_byte_off, h->b.buf[B::RBYTE], size_t(h->n_reads + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return DM_OK;
}

// the scan of the stage on its own: values [n + 1] (host) <- the exclusive prefix sums of values [0 .. n) and their total, computed on the device
int dm_xy_scan(dm_xyrows* h, int64_t* values, int64_t n) {
    if (!h || !values || n <= 0 || n > (int64_t(1) << 40)) return fail(DM_EINVAL, "dm_xy_scan: null argument or no value");
    HIP_TRY(hipSetDevice(h->device));
    int rc = h->b.ensure(dm_xyrows::LEN, size_t(n + 1) * 8);
    if (rc) return rc;
    long long* d = static_cast<long long*>(h->b.buf[dm_xyrows::LEN]);
    HIP_TRY(hipMemcpyAsync(d, values, size_t(n) * 8, hipMemcpyHostToDevice, h->stream));
    if ((rc = xyk::scan_in_place(h, d, n)) != DM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(values, d, size_t(n + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return DM_OK;
}

int dm_xy_times(dm_xyrows* h, double* keep_ms, double* text_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (keep_ms) *keep_ms = 0.0;
    if (text_ms) *text_ms = 0.0;
    if (!h->timed) return DM_OK;                                     // no batch, or one that took the host path
    float a = 0.0f, b = 0.0f;
    HIP_TRY(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
    if (keep_ms) *keep_ms = double(a);
    if (text_ms) *text_ms = double(b);
    return DM_OK;
}

}  // extern "C"
