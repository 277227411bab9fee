// xyparse.hip.inc — predict, device part (part of offline.hip): the text of one .xy file -> its table, and the rows
// whose windows are classified.  The inverse of xyrows.hip.inc (which writes this text) and the device statement of train.getDataFromFile_new
// (np.loadtxt + the selection of myMultiBiRNN.py:306-343).
//
// The text: lines of ten fields `-?[0-9]+(\.[0-9]+)?` with at most 15 digit characters each, one space between fields, '\n' after the tenth (the
// host appends a missing last one).  Anything else - nan, inf, an exponent, '+', a tab, two spaces, '\r', an empty line, '#', nine or eleven
// fields, 16 digits, '.5', '5.' - marks its line and the file is loaded on the host instead (xyload.py: np.loadtxt): the result is np.loadtxt's
// either way.
// A field's value (parse_row, compiled for both sides: dm_xyload_parse_host runs it on the host): the digits as an integer m < 10^15 < 2^53, the
// power 10^k of its k decimals as an integer <= 10^15 - both exact as doubles - ONE IEEE division, the sign last (-0.000 is -0.0), the cast to
// float.  m / 10^k with exact operands is the correctly rounded double of the decimal (Clinger's exact case), i.e. what strtod and np.loadtxt
// produce before their cast; contraction is off so that the division stays a division.
// The text is split into lines by textlines.hip.inc (xlk::split: the newline kernels and the 64-bit scan), then
//   xl_parse_kernel   one row per lane: parse_row -> head [R][3] (position, two labels), feats [R][7], a status byte
//   xlk::first_bad    the smallest row with a status byte set (-1: none)
// Selection (xl_want_kernel, the scan, xl_compact_kernel): a row is wanted unless both labels are below 0.01f; under kind '-' not if
// lo < int(position) < hi, under '+' only then (the float32 position truncated, as the reference's astype(int)); the wanted rows in ascending
// order -> centre int32 [n] and label u8 [n] (1: int(column 2) == 1, myMultiBiRNN.py:407); a wanted row with fewer than 10 rows to an edge of the
// file raises its status byte (xl_first_kernel: the first of them).  NaN cannot come out of parse_row, so the loader's NaN rule lives on the host
// path only.  dm_xyload_select_host runs the same three rules (row_wanted, the edge, row_label) on a host table.
// dm_xyload_classify: dm_predict_read_at on the resident table and centres, xl_prob1_kernel gathers column 1 of the probabilities; class,
// probability and label come back as three plain copies, 6 bytes per window.
#pragma once
#include "host.h"
#include "xyrows.hip.inc"
#include "textlines.hip.inc"
#include "bedline.inc"                                  // for_each_line

namespace xlk {

constexpr int MAX_DIGITS = 15;
constexpr int HALF = DM_WINDOW / 2;

// One line p[0 .. n) (without its '\n') -> ten floats; false: outside the grammar (out is then unspecified).
__host__ __device__ inline bool parse_row(const char* __restrict__ p, const long long n, float* __restrict__ out) {
#pragma clang fp contract(off)
    long long i = 0;
    for (int f = 0; f < 10; ++f) {
        const bool neg = i < n && p[i] == '-';
        if (neg) ++i;
        unsigned long long m = 0, scale = 1;
        int digits = 0, whole = 0, decimals = 0;
        bool point = false;
        for (; i < n; ++i) {
            const char c = p[i];
            if (c >= '0' && c <= '9') {
                if (++digits > MAX_DIGITS) return false;
                m = m * 10ull + (unsigned long long)(c - '0');
                if (point) {
                    scale *= 10ull;
                    ++decimals;
                } else {
                    ++whole;
                }
            } else if (c == '.' && !point && whole > 0) {
                point = true;
            } else {
                break;
            }
        }
        if (whole == 0 || (point && decimals == 0)) return false;
        if (f < 9 ? !(i < n && p[i] == ' ') : i != n) return false;
        ++i;
        const double v = double(m) / double(scale);
        out[f] = float(neg ? -v : v);
    }
    return true;
}

__global__ __launch_bounds__(THREADS) void xl_parse_kernel(const char* __restrict__ text, const long long* __restrict__ start, const long long n_rows,
                                                          float* __restrict__ head, float* __restrict__ feats, unsigned char* __restrict__ status) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const long long b = start[r], e = start[r + 1] - 1;              // text[e] is the line's '\n'
    float v[10];
    const bool ok = parse_row(text + b, e - b, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) head[3 * r + c] = ok ? v[c] : 0.0f;
#pragma unroll
    for (int c = 0; c < DM_NFEAT; ++c) feats[DM_NFEAT * r + c] = ok ? v[3 + c] : 0.0f;
    status[r] = ok ? 0 : 1;
}

__host__ __device__ inline bool row_wanted(const float* __restrict__ h /* position, label 0, label 1 */, const int kind, const long long lo, const long long hi) {
    bool wanted = !(h[1] < 0.01f && h[2] < 0.01f);
    if (kind != 0) {
        const long long ipos = (long long)h[0];
        const bool inside = lo < ipos && ipos < hi;
        wanted = wanted && (kind < 0 ? !inside : inside);
    }
    return wanted;
}

// 1: int(column 2) == 1 (myMultiBiRNN.py:407 on labels.astype(int))
__host__ __device__ inline unsigned char row_label(const float* __restrict__ h) { return (long long)h[2] == 1 ? 1 : 0; }

__global__ __launch_bounds__(THREADS) void xl_want_kernel(const float* __restrict__ head, const long long n_rows, const int kind, const long long lo, const long long hi,
                                                         long long* __restrict__ want, unsigned char* __restrict__ status) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const bool w = row_wanted(head + 3 * r, kind, lo, hi);
    want[r] = w ? 1 : 0;
    status[r] = w && (r < HALF || r + HALF >= n_rows) ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void xl_compact_kernel(const float* __restrict__ head, const long long* __restrict__ scan, const long long n_rows,
                                                            int* __restrict__ centre, unsigned char* __restrict__ label) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_rows) return;
    const long long at = scan[r];
    if (scan[r + 1] == at) return;
    centre[at] = int(r);
    label[at] = row_label(head + 3 * r);
}

// column 1 of prob [n][2] -> prob1 [n]: what `predict` downloads is one contiguous copy
__global__ __launch_bounds__(THREADS) void xl_prob1_kernel(const float* __restrict__ prob, const long long n, float* __restrict__ prob1) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) prob1[i] = prob[2 * i + 1];
}

}  // namespace xlk

struct dm_xyload {
    dm_xyrows* xy = nullptr;                            // stream, the scan and its block sums
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    enum { HEAD = xlk::N_SPLIT, FEATS, WANT, CENTRE, LABEL, PROB, PROB1, CLS, N_BUF };
    DevBufs<N_BUF> b{"dm_xyload"};
    int64_t n_rows = -1, n = -1;                        // of the table on the device (-1: none) and of its selection (-1: none)
    bool flagged = false;                               // the last text held a line outside the grammar: its table is not to be used
    bool parse_timed = false, select_timed = false;
};

namespace xlk {

constexpr int64_t MAX_ROWS = 0x7fffffffLL - HALF;                     // centre is int32

int table_buffers(dm_xyload* h, int64_t n_rows) {
    int rc;
    if ((rc = h->b.ensure(dm_xyload::HEAD, size_t(n_rows) * 12)) != DM_OK) return rc;
    if ((rc = h->b.ensure(dm_xyload::FEATS, size_t(n_rows) * 4 * DM_NFEAT)) != DM_OK) return rc;
    return h->b.ensure(STATUS, size_t(n_rows));
}

}  // namespace xlk

extern "C" {

int dm_xyload_tile_bytes(void) { return xlk::TILE; }
int dm_xyload_scan_block(void) { return xyk::SCAN_TILE; }

void dm_xyload_destroy(dm_xyload* h) {
    if (!h) return;
    if (h->xy) (void)hipSetDevice(h->xy->device);
    h->b.release();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    dm_xy_destroy(h->xy);
    delete h;
}

dm_xyload* dm_xyload_create(int device) {
    dm_xyrows* xy = dm_xy_create(device);
    if (!xy) return nullptr;
    dm_xyload* h = new dm_xyload;
    h->xy = xy;
    for (hipEvent_t& e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            fail(DM_EDEVICE, "dm_xyload_create: events on device %d", device);
            dm_xyload_destroy(h);
            return nullptr;
        }
    return h;
}

int64_t dm_xyload_parse_host(const char* text, int64_t n_bytes, float* table, int64_t cap_rows, int32_t* flag, int64_t* first_bad_line) {
    if (n_bytes < 0 || (n_bytes > 0 && !text) || cap_rows < 0 || (cap_rows > 0 && !table)) return fail(DM_EINVAL, "dm_xyload_parse_host: null argument");
    int64_t bad = 0;
    const int64_t rows = bed::for_each_line(text, n_bytes, &bad, [&](const char* line, const int64_t len, const int64_t row) {
        float v[10];
        const bool ok = xlk::parse_row(line, len, v);
        if (row < cap_rows)
            for (int c = 0; c < 10; ++c) table[10 * row + c] = ok ? v[c] : 0.0f;
        return ok;
    });
    if (flag) *flag = bad != 0;
    if (first_bad_line) *first_bad_line = bad ? bad : -1;
    return rows;
}

// the selection on the host, with the routines the kernels run (row_wanted, the edge rule, the label rule)
int64_t dm_xyload_select_host(const float* table, int64_t n_rows, int kind, int64_t lo, int64_t hi, int32_t* centre, uint8_t* label, int64_t cap, int64_t* short_row) {
    if (short_row) *short_row = -1;
    if (n_rows < 0 || n_rows > xlk::MAX_ROWS || (n_rows > 0 && !table) || cap < 0 || (cap > 0 && (!centre || !label)))
        return fail(DM_EINVAL, "dm_xyload_select_host: null argument or %lld rows", (long long)n_rows);
    if (kind != 0 && kind != '-' && kind != '+') return fail(DM_EINVAL, "dm_xyload_select_host: kind %d (0, '-' or '+')", kind);
    const int k = kind == 0 ? 0 : (kind == '-' ? -1 : 1);
    int64_t n = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (!xlk::row_wanted(table + 10 * r, k, lo, hi)) continue;
        if (r < xlk::HALF || r + xlk::HALF >= n_rows) {
            if (short_row) *short_row = r;
            return fail(DM_EINVAL, "dm_xyload_select_host: labelled row %lld is closer than %d rows to the edge of the table (%lld rows): no whole window", (long long)r,
                        xlk::HALF, (long long)n_rows);
        }
        if (n < cap) {
            centre[n] = int32_t(r);
            label[n] = xlk::row_label(table + 10 * r);
        }
        ++n;
    }
    return n;
}

int dm_xyload_parse(dm_xyload* h, const char* text, int64_t n_bytes, int64_t* n_rows, int32_t* flag, int64_t* first_bad_line) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->n_rows = h->n = -1;
    h->flagged = h->parse_timed = h->select_timed = false;
    if (n_rows) *n_rows = 0;
    if (flag) *flag = 0;
    if (first_bad_line) *first_bad_line = -1;
    HIP_TRY(hipSetDevice(h->xy->device));
    using B = dm_xyload;
    int rc;
    long long rows = 0;
    if ((rc = xlk::split(h->xy, h->b, text, n_bytes, xlk::MAX_ROWS, "dm_xyload_parse", "rows", h->ev[0], &rows)) != DM_OK) return rc;
    if ((rc = xlk::table_buffers(h, rows)) != DM_OK) return rc;
    if (rows == 0) {                                                 // an empty file: a table of no rows
        h->n_rows = 0;
        return DM_OK;
    }
    hipStream_t s = h->xy->stream;
    hipLaunchKernelGGL(xlk::xl_parse_kernel, dim3(unsigned((rows + xlk::THREADS - 1) / xlk::THREADS)), dim3(xlk::THREADS), 0, s, h->b.ptr<const char>(xlk::TEXT),
                       h->b.ptr<const long long>(xlk::START), rows, h->b.ptr<float>(B::HEAD), h->b.ptr<float>(B::FEATS), h->b.ptr<unsigned char>(xlk::STATUS));
    HIP_TRY(hipGetLastError());
    if ((rc = xlk::first_bad(h->xy, h->b, rows)) != DM_OK) return rc;
    HIP_TRY(hipEventRecord(h->ev[1], s));
    long long first = -1;
    HIP_TRY(hipMemcpyAsync(&first, h->b.buf[xlk::OUT], 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->n_rows = rows;
    h->flagged = first >= 0;
    h->parse_timed = true;
    if (n_rows) *n_rows = rows;
    if (flag) *flag = first >= 0;
    if (first_bad_line) *first_bad_line = first >= 0 ? first + 1 : -1;
    return DM_OK;
}

int dm_xyload_set_table(dm_xyload* h, const float* table, int64_t n_rows) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->n_rows = h->n = -1;
    h->flagged = h->parse_timed = h->select_timed = false;
    if (n_rows < 0 || n_rows > xlk::MAX_ROWS || (n_rows > 0 && !table)) return fail(DM_EINVAL, "dm_xyload_set_table: %lld rows", (long long)n_rows);
    HIP_TRY(hipSetDevice(h->xy->device));
    int rc = xlk::table_buffers(h, n_rows);
    if (rc) return rc;
    std::vector<float> head(size_t(n_rows) * 3), feats(size_t(n_rows) * DM_NFEAT);
    for (int64_t r = 0; r < n_rows; ++r) {
        std::memcpy(&head[size_t(r) * 3], table + 10 * r, 12);
        std::memcpy(&feats[size_t(r) * DM_NFEAT], table + 10 * r + 3, 4 * DM_NFEAT);
    }
    if (n_rows > 0) {
        HIP_TRY(hipMemcpyAsync(h->b.buf[dm_xyload::HEAD], head.data(), head.size() * 4, hipMemcpyHostToDevice, h->xy->stream));
        HIP_TRY(hipMemcpyAsync(h->b.buf[dm_xyload::FEATS], feats.data(), feats.size() * 4, hipMemcpyHostToDevice, h->xy->stream));
        HIP_TRY(hipStreamSynchronize(h->xy->stream));
    }
    h->n_rows = n_rows;
    return DM_OK;
}

int64_t dm_xyload_select(dm_xyload* h, int kind, int64_t lo, int64_t hi, int64_t* short_row) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->n = -1;
    h->select_timed = false;
    if (short_row) *short_row = -1;
    if (h->n_rows < 0) return fail(DM_ESTATE, "dm_xyload_select: no table");
    if (h->flagged) return fail(DM_ESTATE, "dm_xyload_select: the text was outside the device grammar; give the host's table with dm_xyload_set_table");
    if (kind != 0 && kind != '-' && kind != '+') return fail(DM_EINVAL, "dm_xyload_select: kind %d (0, '-' or '+')", kind);
    const int64_t rows = h->n_rows;
    if (rows == 0) {
        h->n = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(h->xy->device));
    using B = dm_xyload;
    int rc;
    if ((rc = h->b.ensure(B::WANT, size_t(rows + 1) * 8)) != DM_OK) return rc;
    hipStream_t s = h->xy->stream;
    const float* d_head = h->b.ptr<float>(B::HEAD);
    long long* d_want = h->b.ptr<long long>(B::WANT);
    const dim3 row_grid{unsigned((rows + xlk::THREADS - 1) / xlk::THREADS)}, block{xlk::THREADS};
    HIP_TRY(hipEventRecord(h->ev[2], s));
    hipLaunchKernelGGL(xlk::xl_want_kernel, row_grid, block, 0, s, d_head, (long long)rows, kind == 0 ? 0 : (kind == '-' ? -1 : 1), (long long)lo, (long long)hi, d_want,
                       h->b.ptr<unsigned char>(xlk::STATUS));
    HIP_TRY(hipGetLastError());
    if ((rc = xlk::first_bad(h->xy, h->b, rows)) != DM_OK) return rc;
    if ((rc = xyk::scan_in_place(h->xy, d_want, rows)) != DM_OK) return rc;
    long long out[2] = {-1, 0};
    HIP_TRY(hipMemcpyAsync(&out[0], h->b.buf[xlk::OUT], 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&out[1], d_want + rows, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out[0] >= 0) {
        if (short_row) *short_row = out[0];
        return fail(DM_EINVAL, "dm_xyload_select: labelled row %lld is closer than %d rows to the edge of the table (%lld rows): no whole window", out[0], xlk::HALF,
                    (long long)rows);
    }
    const int64_t n = out[1];
    if (n < 0 || n > rows) return fail(DM_ESTATE, "dm_xyload_select: %lld of %lld rows", (long long)n, (long long)rows);
    if (n > 0) {
        if ((rc = h->b.ensure(B::CENTRE, size_t(n) * 4)) != DM_OK) return rc;
        if ((rc = h->b.ensure(B::LABEL, size_t(n))) != DM_OK) return rc;
        hipLaunchKernelGGL(xlk::xl_compact_kernel, row_grid, block, 0, s, d_head, d_want, (long long)rows, h->b.ptr<int>(B::CENTRE), h->b.ptr<unsigned char>(B::LABEL));
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(h->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    h->n = n;
    h->select_timed = true;
    return n;
}

int dm_xyload_set_selection(dm_xyload* h, const int32_t* centre, const uint8_t* label, int64_t n) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->n = -1;
    h->select_timed = false;
    if (h->n_rows < 0) return fail(DM_ESTATE, "dm_xyload_set_selection: no table");
    if (n < 0 || n > h->n_rows || (n > 0 && (!centre || !label))) return fail(DM_EINVAL, "dm_xyload_set_selection: %lld rows of %lld", (long long)n, (long long)h->n_rows);
    for (int64_t i = 0; i < n; ++i)
        if (centre[i] < xlk::HALF || centre[i] >= h->n_rows - xlk::HALF)
            return fail(DM_EINVAL, "dm_xyload_set_selection: centre row %d +-%d outside the %lld rows", centre[i], xlk::HALF, (long long)h->n_rows);
    HIP_TRY(hipSetDevice(h->xy->device));
    if (n > 0) {
        int rc;
        if ((rc = h->b.ensure(dm_xyload::CENTRE, size_t(n) * 4)) != DM_OK) return rc;
        if ((rc = h->b.ensure(dm_xyload::LABEL, size_t(n))) != DM_OK) return rc;
        HIP_TRY(hipMemcpyAsync(h->b.buf[dm_xyload::CENTRE], centre, size_t(n) * 4, hipMemcpyHostToDevice, h->xy->stream));
        HIP_TRY(hipMemcpyAsync(h->b.buf[dm_xyload::LABEL], label, size_t(n), hipMemcpyHostToDevice, h->xy->stream));
        HIP_TRY(hipStreamSynchronize(h->xy->stream));
    }
    h->n = n;
    return DM_OK;
}

int dm_xyload_device(dm_xyload* h, const float** d_feats, const int32_t** d_centre, int64_t* n_rows, int64_t* n) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (h->n_rows < 0) return fail(DM_ESTATE, "dm_xyload_device: no table");
    if (d_feats) *d_feats = h->b.ptr<const float>(dm_xyload::FEATS);
    if (d_centre) *d_centre = h->n > 0 ? h->b.ptr<const int32_t>(dm_xyload::CENTRE) : nullptr;
    if (n_rows) *n_rows = h->n_rows;
    if (n) *n = h->n;
    return DM_OK;
}

int dm_xyload_fetch(dm_xyload* h, float* feats, float* head, int32_t* centre, uint8_t* label) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (h->n_rows < 0) return fail(DM_ESTATE, "dm_xyload_fetch: no table");
    if ((centre || label) && h->n < 0) return fail(DM_ESTATE, "dm_xyload_fetch: no selection");
    HIP_TRY(hipSetDevice(h->xy->device));
    hipStream_t s = h->xy->stream;
    using B = dm_xyload;
    if (feats && h->n_rows > 0) HIP_TRY(hipMemcpyAsync(feats, h->b.buf[B::FEATS], size_t(h->n_rows) * 4 * DM_NFEAT, hipMemcpyDeviceToHost, s));
    if (head && h->n_rows > 0) HIP_TRY(hipMemcpyAsync(head, h->b.buf[B::HEAD], size_t(h->n_rows) * 12, hipMemcpyDeviceToHost, s));
    if (centre && h->n > 0) HIP_TRY(hipMemcpyAsync(centre, h->b.buf[B::CENTRE], size_t(h->n) * 4, hipMemcpyDeviceToHost, s));
    if (label && h->n > 0) HIP_TRY(hipMemcpyAsync(label, h->b.buf[B::LABEL], size_t(h->n), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

int dm_xyload_classify(dm_xyload* h, dm_model* m, float* prob1, uint8_t* cls, uint8_t* label) {
    if (!h || !m) return fail(DM_EINVAL, "null handle");
    if (h->n_rows < 0 || h->n < 0) return fail(DM_ESTATE, "dm_xyload_classify: no selection");
    if (model_device(m) != h->xy->device) return fail(DM_EINVAL, "dm_xyload_classify: the model is on device %d, the table on device %d", model_device(m), h->xy->device);
    if (h->n == 0) return DM_OK;
    if (!prob1 || !cls) return fail(DM_EINVAL, "dm_xyload_classify: null output");
    const int64_t n = h->n;
    using B = dm_xyload;
    int rc;
    if ((rc = h->b.ensure(B::PROB, size_t(n) * 8)) != DM_OK) return rc;
    if ((rc = h->b.ensure(B::PROB1, size_t(n) * 4)) != DM_OK) return rc;
    if ((rc = h->b.ensure(B::CLS, size_t(n))) != DM_OK) return rc;
    float* d_prob = h->b.ptr<float>(B::PROB);
    if ((rc = dm_predict_read_at(m, h->b.ptr<const float>(B::FEATS), h->n_rows, h->b.ptr<const int32_t>(B::CENTRE), n, d_prob, h->b.ptr<uint8_t>(B::CLS))) != DM_OK)
        return rc;
    if ((rc = dm_model_sync(m)) != DM_OK) return rc;                 // a model in asynchronous mode has only queued the launch
    hipStream_t s = h->xy->stream;
    hipLaunchKernelGGL(xlk::xl_prob1_kernel, dim3(unsigned((n + xlk::THREADS - 1) / xlk::THREADS)), dim3(xlk::THREADS), 0, s, d_prob, (long long)n, h->b.ptr<float>(B::PROB1));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(prob1, h->b.buf[B::PROB1], size_t(n) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cls, h->b.buf[B::CLS], size_t(n), hipMemcpyDeviceToHost, s));
    if (label) HIP_TRY(hipMemcpyAsync(label, h->b.buf[B::LABEL], size_t(n), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

int dm_xyload_times(dm_xyload* h, double* parse_ms, double* select_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (parse_ms) *parse_ms = 0.0;
    if (select_ms) *select_ms = 0.0;
    float a = 0.0f;
    if (h->parse_timed && parse_ms) {
        HIP_TRY(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
        *parse_ms = double(a);
    }
    if (h->select_timed && select_ms) {
        HIP_TRY(hipEventElapsedTime(&a, h->ev[2], h->ev[3]));
        *select_ms = double(a);
    }
    return DM_OK;
}

}  // extern "C"

// ---- the resident set: what dm_xyload holds after a file's load, for many files at once -------------------------------------------
// `train --validate` scores the same held-out files at every checkpoint.  A loaded file that has windows becomes a SEGMENT: its feature rows
// [R][7], its centres int32 [n] (relative to the segment's first row) and its labels u8 [n], appended to three growing device blocks by
// device-to-device copies on the set's stream - 28 bytes per row + 5 per window, no text, no head columns, no scan scratch.  A segment is
// classified exactly as dm_xyload_classify classifies its file (dm_predict_read_at on the segment's rows and centres, then xl_prob1_kernel),
// so the results are the loader's byte for byte, and DM_ERANGE is a segment's own.
struct dm_xyset {
    int device = 0;
    hipStream_t stream = nullptr;
    float* feats = nullptr;                             // [cap_rows][7]
    int32_t* centre = nullptr;                          // [cap_centre], relative to the segment's first row
    uint8_t* label = nullptr;                           // [cap_label]
    int64_t cap_rows = 0, cap_centre = 0, cap_label = 0;
    std::vector<int64_t> row_off{0}, win_off{0};        // segment s = rows [row_off[s], row_off[s+1]), windows [win_off[s], win_off[s+1])
    float *prob = nullptr, *prob1 = nullptr;            // scratch of the largest segment classified so far
    uint8_t* cls = nullptr;
    int64_t cap_out = 0;
    // the gather by window id (xygather.hip.inc): the segment table on the device and dm_xyset_gather's scratch
    long long* d_off = nullptr;                         // win_off [S + 1], row_off [S + 1] of the d_off_segs segments it was uploaded for
    size_t cap_off = 0;
    int64_t d_off_segs = -1;
    std::vector<long long> off_host;
    enum { G_IDS, G_X, N_GATHER };
    DevBufs<N_GATHER> gather{"dm_xyset_gather"};            // ids or x of a host caller
    void* g_bad = nullptr;
};

namespace xlk {

// a block of `have` used and `cap` allocated elements of `elem` bytes is to hold `need`: at least doubled, the used part copied on the stream
template <class T>
int set_grow(dm_xyset* s, T*& block, int64_t& cap, int64_t have, int64_t need, size_t elem) {
    if (need <= cap && block) return DM_OK;
    const int64_t want = std::max<int64_t>(need, 2 * cap);
    T* fresh = nullptr;
    if (hipMalloc(&fresh, size_t(want) * elem + 256) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DM_ENOMEM, "dm_xyset: hipMalloc(%zu) failed", size_t(want) * elem + 256);
    }
    if (block && have > 0 &&
        (hipMemcpyAsync(fresh, block, size_t(have) * elem, hipMemcpyDeviceToDevice, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess)) {
        (void)hipGetLastError();
        (void)hipFree(fresh);
        return fail(DM_EDEVICE, "dm_xyset: moving %lld elements to a larger block failed", (long long)have);
    }
    if (block) (void)hipFree(block);
    block = fresh;
    cap = want;
    return DM_OK;
}

}  // namespace xlk

extern "C" {

void dm_xyset_destroy(dm_xyset* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (void* b : {(void*)s->feats, (void*)s->centre, (void*)s->label, (void*)s->prob, (void*)s->prob1, (void*)s->cls, (void*)s->d_off, s->g_bad})
        if (b) (void)hipFree(b);
    s->gather.release();
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

dm_xyset* dm_xyset_create(int device, int64_t initial_rows) {
    if (initial_rows < 0 || initial_rows > xlk::MAX_ROWS) {
        fail(DM_EINVAL, "dm_xyset_create: %lld initial rows", (long long)initial_rows);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_xyset_create: device %d", device);
        return nullptr;
    }
    dm_xyset* s = new dm_xyset;
    s->device = device;
    const int64_t rows = std::max<int64_t>(initial_rows, 1);
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_xyset_create: stream on device %d", device);
        s->stream = nullptr;
        dm_xyset_destroy(s);
        return nullptr;
    }
    // one window in eight rows is the expectation the first blocks are sized by; every block grows on its own
    if (xlk::set_grow(s, s->feats, s->cap_rows, 0, rows, sizeof(float) * DM_NFEAT) != DM_OK ||
        xlk::set_grow(s, s->centre, s->cap_centre, 0, rows / 8 + 1, sizeof(int32_t)) != DM_OK ||
        xlk::set_grow(s, s->label, s->cap_label, 0, rows / 8 + 1, 1) != DM_OK) {
        std::string keep = g_err;
        dm_xyset_destroy(s);
        g_err = keep;
        return nullptr;
    }
    return s;
}

int dm_xyset_append(dm_xyset* s, dm_xyload* h) {
    if (!s || !h) return fail(DM_EINVAL, "null handle");
    if (h->n_rows < 0 || h->n < 0) return fail(DM_ESTATE, "dm_xyset_append: the loader holds no selection");
    if (h->xy->device != s->device) return fail(DM_EINVAL, "dm_xyset_append: the loader is on device %d, the set on device %d", h->xy->device, s->device);
    if (h->n == 0) return DM_OK;                                     // a file without a window: no segment
    if (h->n > h->n_rows) return fail(DM_ESTATE, "dm_xyset_append: %lld windows of %lld rows", (long long)h->n, (long long)h->n_rows);
    HIP_TRY(hipSetDevice(s->device));
    const int64_t rows = s->row_off.back(), wins = s->win_off.back(), R = h->n_rows, n = h->n;
    int rc;
    if ((rc = xlk::set_grow(s, s->feats, s->cap_rows, rows, rows + R, sizeof(float) * DM_NFEAT)) != DM_OK) return rc;
    if ((rc = xlk::set_grow(s, s->centre, s->cap_centre, wins, wins + n, sizeof(int32_t))) != DM_OK) return rc;
    if ((rc = xlk::set_grow(s, s->label, s->cap_label, wins, wins + n, 1)) != DM_OK) return rc;
    using B = dm_xyload;
    HIP_TRY(hipMemcpyAsync(s->feats + rows * DM_NFEAT, h->b.buf[B::FEATS], size_t(R) * 4 * DM_NFEAT, hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->centre + wins, h->b.buf[B::CENTRE], size_t(n) * 4, hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->label + wins, h->b.buf[B::LABEL], size_t(n), hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));                        // the loader may take its next file, or be destroyed
    s->row_off.push_back(rows + R);
    s->win_off.push_back(wins + n);
    return DM_OK;
}

int64_t dm_xyset_segments(dm_xyset* s, int64_t* rows, int64_t* windows, int64_t cap) {
    if (!s) return fail(DM_EINVAL, "null handle");
    const int64_t k = int64_t(s->row_off.size()) - 1;
    if (cap < 0 || (cap > 0 && rows == nullptr && windows == nullptr)) return fail(DM_EINVAL, "dm_xyset_segments: null output");
    for (int64_t i = 0; i < k && i < cap; ++i) {
        if (rows) rows[i] = s->row_off[i + 1] - s->row_off[i];
        if (windows) windows[i] = s->win_off[i + 1] - s->win_off[i];
    }
    return k;
}

int64_t dm_xyset_bytes(dm_xyset* s) {
    if (!s) return fail(DM_EINVAL, "null handle");
    return s->row_off.back() * 4 * DM_NFEAT + s->win_off.back() * 5;
}

int dm_xyset_classify(dm_xyset* s, dm_model* m, int64_t segment, float* prob1, uint8_t* cls, uint8_t* label) {
    if (!s || !m) return fail(DM_EINVAL, "null handle");
    if (segment < 0 || segment + 1 >= int64_t(s->row_off.size())) return fail(DM_EINVAL, "dm_xyset_classify: segment %lld of %lld", (long long)segment, (long long)s->row_off.size() - 1);
    if (model_device(m) != s->device) return fail(DM_EINVAL, "dm_xyset_classify: the model is on device %d, the set on device %d", model_device(m), s->device);
    if (!prob1 || !cls) return fail(DM_EINVAL, "dm_xyset_classify: null output");
    const int64_t row0 = s->row_off[segment], R = s->row_off[segment + 1] - row0, win0 = s->win_off[segment], n = s->win_off[segment + 1] - win0;
    HIP_TRY(hipSetDevice(s->device));
    if (n > s->cap_out) {
        for (void* b : {(void*)s->prob, (void*)s->prob1, (void*)s->cls})
            if (b) (void)hipFree(b);
        s->prob = s->prob1 = nullptr;
        s->cls = nullptr;
        s->cap_out = 0;
        const int64_t want = n + (n >> 2) + 64;
        if (hipMalloc(&s->prob, size_t(want) * 8) != hipSuccess || hipMalloc(&s->prob1, size_t(want) * 4) != hipSuccess || hipMalloc(&s->cls, size_t(want)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(DM_ENOMEM, "dm_xyset_classify: hipMalloc for %lld windows failed", (long long)want);
        }
        s->cap_out = want;
    }
    int rc;
    if ((rc = dm_predict_read_at(m, s->feats + row0 * DM_NFEAT, R, s->centre + win0, n, s->prob, s->cls)) != DM_OK) return rc;
    if ((rc = dm_model_sync(m)) != DM_OK) return rc;                 // a model in asynchronous mode has only queued the launch
    hipLaunchKernelGGL(xlk::xl_prob1_kernel, dim3(unsigned((n + xlk::THREADS - 1) / xlk::THREADS)), dim3(xlk::THREADS), 0, s->stream, s->prob, (long long)n, s->prob1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(prob1, s->prob1, size_t(n) * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(cls, s->cls, size_t(n), hipMemcpyDeviceToHost, s->stream));
    if (label) HIP_TRY(hipMemcpyAsync(label, s->label + win0, size_t(n), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return DM_OK;
}

}  // extern "C"
