// bedmerge.hip.inc — `merge`, device part (part of offline.hip): the BED files of several runs of one contig -> their sums in two dm_summary
// tables -> the merged text of DeepMod_tools/sum_chr_mod.py.
//   readbed2 (:37-46)    bm_parse_kernel    one line per lane (bmk::parse_line, bedmerge.inc) -> position, strand, coverage, modified, a status byte;
//                                           the largest position and coverage of the text (one integer atomic max per wave)
//   mergeMod (:48-54)    bm_add_kernel      a record -> int32 atomic adds into cov and mod of its strand's table, +1 into touch
//   save_mod (:56-66)    the tiled writer of textout.hip.inc (txo::Run) on bmk::Emitter: the lines of a position from the four sum tables; a tile
//                        with a sum outside 0 <= mod <= cov is counted, and format_begin refuses the contig
// The text of a file is split into lines by textlines.hip.inc (xlk::split).  The grammar and the line are stated in bedmerge.inc; a text with a line outside the grammar adds nothing (first line reported), and the caller hands its own parse over through
// dm_bedmerge_add_records.
// Exactness and determinism.  Every sum is an int32 integer: additions commute, so the order the atomics land in does not matter.  The guard of
// siteperf keeps the sums in range: the largest coverages of the texts of a contig sum to < 2^31 (checked BEFORE a text's adds; duplicates of a key
// inside one file are summed too, as merge.merge_beds sums them - a sum that left 0 <= mod <= cov through them is refused by format_begin).  The
// format has no atomics: a line's offset is its tile's scanned offset + the block scan of the bytes of the lanes before it, a function of the tables
// alone, and every output byte has one writer.  Two runs give identical bytes.
// The tables belong to the caller (dm_summary handles, the ones dm_cluster_sites takes) and have a stream of their own: dm_summary_sync before this
// handle's stream touches them, a stream synchronisation of this handle before the call returns.
#pragma once
#include "host.h"
#include "blockscan.hip.inc"
#include "xyrows.hip.inc"
#include "textlines.hip.inc"
#include "textout.hip.inc"
#include "bedmerge.inc"

namespace bmk {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 1024;
enum { S_MAXPOS, S_MAXCOV, S_BADSUM, N_STAT };

__global__ __launch_bounds__(THREADS) void bm_parse_kernel(const char* __restrict__ text, const long long* __restrict__ start, const long long n_rows, const Name name,
                                                          const long long limit, int* __restrict__ pos, int* __restrict__ cov, int* __restrict__ mod,
                                                          unsigned char* __restrict__ strand, unsigned char* __restrict__ status, unsigned long long* __restrict__ stat) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    long long mp = 0, mc = 0;
    if (r < n_rows) {
        const long long b = start[r], e = start[r + 1] - 1;          // text[e] is the line's '\n'
        Rec v = {0, 0, 0, 0};
        const bool ok = parse_line(text + b, e - b, name, limit, v);
        pos[r] = ok ? v.pos : 0;
        cov[r] = ok ? v.cov : 0;
        mod[r] = ok ? v.mod : 0;
        strand[r] = ok ? v.strand : 0;
        status[r] = ok ? 0 : 1;
        if (ok) {
            mp = v.pos;
            mc = v.cov;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        mp = max(mp, __shfl_down(mp, d, 64));
        mc = max(mc, __shfl_down(mc, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (mp > 0) atomicMax(stat + S_MAXPOS, (unsigned long long)mp);
        if (mc > 0) atomicMax(stat + S_MAXCOV, (unsigned long long)mc);
    }
}

// tables: touch | cov | mod of `length` positions each; every pos[i] < length (parse_line's limit / the check of add_records)
__global__ __launch_bounds__(THREADS) void bm_add_kernel(const int* __restrict__ pos, const int* __restrict__ cov, const int* __restrict__ mod,
                                                        const unsigned char* __restrict__ strand, const long long n, int* __restrict__ plus, int* __restrict__ minus,
                                                        const long long length) {
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * THREADS) {
        const long long q = pos[i];
        if (q < 0 || q >= length) continue;
        int* t = (strand[i] & 1) ? minus : plus;
        atomicAdd(&t[q], 1);
        atomicAdd(&t[length + q], cov[i]);
        atomicAdd(&t[2 * length + q], mod[i]);
    }
}

}  // namespace bmk

struct dm_bedmerge {
    dm_xyrows* xy = nullptr;                            // stream, the scan and its block sums
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};          // parse, add: begin / end
    enum { POS = xlk::N_SPLIT, COV, MOD, STRAND, STAT, N_BUF };
    DevBufs<N_BUF> b{"dm_bedmerge"};
    dm_summary *plus = nullptr, *minus = nullptr;       // the open contig's tables (null: none), the caller's
    bool fixed = false;                                 // the table length is the contig's: a line beyond it is outside the grammar
    bmk::Name name = {};
    int64_t n_records = 0;                              // records on the device, of the last add_text / add_records
    int64_t cov_bound = 0;                              // of the open contig: the sum of the largest coverages of its texts
    int64_t lines_seen = 0;
    txo::Run text;                                      // the format in progress, of tables of format_length positions
    int64_t format_length = 0;
    char format_base = 0;
    double parse_ms = 0.0, add_ms = 0.0;
};

namespace bmk {

constexpr int64_t MAX_RECORDS = 0x7fffffffLL;

// the lines of the open contig's tables of `length` positions, as the tables lie now: read for every call, a table that grew has moved
Emitter emitter(const dm_bedmerge* h, const char base, const int64_t length) {
    const int* p = static_cast<const int*>(dm_summary_device_ptr(h->plus));
    const int* m = static_cast<const int*>(dm_summary_device_ptr(h->minus));
    return {h->name, base, p + length, p + 2 * length, m + length, m + 2 * length, h->b.ptr<unsigned long long>(dm_bedmerge::STAT) + S_BADSUM};
}

int record_buffers(dm_bedmerge* h, int64_t n) {
    using B = dm_bedmerge;
    int rc;
    for (int which : {int(B::POS), int(B::COV), int(B::MOD)})
        if ((rc = h->b.ensure(which, size_t(n) * 4)) != DM_OK) return rc;
    for (int which : {int(B::STRAND), int(xlk::STATUS)})
        if ((rc = h->b.ensure(which, size_t(n))) != DM_OK) return rc;
    return DM_OK;
}

// the n records on the device, whose largest position and coverage are max_pos and max_cov -> the tables
int add_device_records(dm_bedmerge* h, int64_t n, int64_t max_pos, int64_t max_cov) {
    using B = dm_bedmerge;
    if (n == 0) return DM_OK;
    if (h->cov_bound + max_cov >= (int64_t(1) << 31))
        return fail(DM_EINVAL, "dm_bedmerge: the largest coverages of this contig's files sum to %lld (2^31 or more): the int32 tables cannot hold them",
                    (long long)(h->cov_bound + max_cov));
    int rc;
    if ((rc = dm_summary_sync(h->plus)) != DM_OK || (rc = dm_summary_sync(h->minus)) != DM_OK) return rc;
    if (!h->fixed && max_pos + 1 > dm_summary_length(h->plus)) {     // the table grows to the largest position + 1 of the file
        if ((rc = dm_summary_grow(h->plus, max_pos + 1)) != DM_OK || (rc = dm_summary_grow(h->minus, max_pos + 1)) != DM_OK) return rc;
    }
    const int64_t length = dm_summary_length(h->plus);
    if (dm_summary_length(h->minus) != length || max_pos >= length)
        return fail(DM_ESTATE, "dm_bedmerge: tables of %lld and %lld positions, largest position %lld", (long long)length, (long long)dm_summary_length(h->minus), (long long)max_pos);
    hipStream_t s = h->xy->stream;
    const dim3 grid{unsigned(std::min<int64_t>((n + THREADS - 1) / THREADS, MAX_BLOCKS))};
    HIP_TRY(hipEventRecord(h->ev[2], s));
    hipLaunchKernelGGL(bm_add_kernel, grid, dim3(THREADS), 0, s, h->b.ptr<const int>(B::POS), h->b.ptr<const int>(B::COV), h->b.ptr<const int>(B::MOD),
                       h->b.ptr<const unsigned char>(B::STRAND), (long long)n, static_cast<int*>(dm_summary_device_ptr(h->plus)),
                       static_cast<int*>(dm_summary_device_ptr(h->minus)), (long long)length);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = add_time(h->ev[2], h->ev[3], h->add_ms)) != DM_OK) return rc;
    h->cov_bound += max_cov;
    h->lines_seen += n;
    h->text.clear();                                                  // a format begun before this add is over
    return DM_OK;
}

}  // namespace bmk

extern "C" {

int dm_bedmerge_tile_positions(void) { return txo::TILE_POS; }

void dm_bedmerge_destroy(dm_bedmerge* h) {
    if (!h) return;
    if (h->xy) {
        (void)hipSetDevice(h->xy->device);
        (void)hipStreamSynchronize(h->xy->stream);
    }
    h->b.release();
    h->text.release();
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    dm_xy_destroy(h->xy);
    delete h;
}

dm_bedmerge* dm_bedmerge_create(int device) {
    dm_xyrows* xy = dm_xy_create(device);
    if (!xy) return nullptr;
    dm_bedmerge* h = new dm_bedmerge;
    h->xy = xy;
    bool ok = h->text.init("dm_bedmerge");
    for (hipEvent_t& e : h->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && h->b.ensure(dm_bedmerge::STAT, bmk::N_STAT * 8) == DM_OK;
    if (!ok) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_bedmerge_create: events or counters on device %d", device);
        dm_bedmerge_destroy(h);
        return nullptr;
    }
    return h;
}

int dm_bedmerge_open(dm_bedmerge* h, dm_summary* plus, dm_summary* minus, const char* contig_name, int fixed_length) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->plus = h->minus = nullptr;
    h->text.clear();
    h->n_records = 0;
    if (!plus || !minus || plus == minus) return fail(DM_EINVAL, "dm_bedmerge_open: two tables, one per strand");
    if (plus->device != h->xy->device || minus->device != h->xy->device) return fail(DM_EINVAL, "dm_bedmerge_open: the tables are on another device than the handle (%d)", h->xy->device);
    const int64_t length = dm_summary_length(plus);
    if (length != dm_summary_length(minus) || length < 1 || length > bmk::MAX_LENGTH)
        return fail(DM_EINVAL, "dm_bedmerge_open: tables of %lld and %lld positions (equal, 1 to 2^31 - 1)", (long long)length, (long long)dm_summary_length(minus));
    if (!bmk::set_name(h->name, contig_name)) return fail(DM_EINVAL, "dm_bedmerge_open: a contig name of 1 to %d printable bytes", bed::MAX_NAME);
    h->plus = plus;
    h->minus = minus;
    h->fixed = fixed_length != 0;
    h->cov_bound = 0;
    h->lines_seen = 0;
    return DM_OK;
}

int64_t dm_bedmerge_parse_host(const char* text, int64_t n_bytes, const char* contig_name, int64_t table_length, int32_t* pos, uint8_t* strand, int32_t* cov, int32_t* mod,
                               int64_t cap, int32_t* flag, int64_t* first_bad_line) {
    if (n_bytes < 0 || (n_bytes > 0 && !text) || cap < 0 || (cap > 0 && (!pos || !strand || !cov || !mod))) return fail(DM_EINVAL, "dm_bedmerge_parse_host: null argument");
    bmk::Name name = {};
    if (!bmk::set_name(name, contig_name)) return fail(DM_EINVAL, "dm_bedmerge_parse_host: a contig name of 1 to %d printable bytes", bed::MAX_NAME);
    const long long limit = (table_length < 0 || table_length > bmk::MAX_LENGTH) ? bmk::MAX_LENGTH : table_length;
    int64_t bad = 0;
    const int64_t rows = bmk::parse_text(text, n_bytes, name, limit, pos, strand, cov, mod, cap, &bad);
    if (flag) *flag = bad != 0;
    if (first_bad_line) *first_bad_line = bad ? bad : -1;
    return rows;
}

int64_t dm_bedmerge_format_host(const char* contig_name, char base, int64_t first_pos, int64_t length, const int32_t* cov_plus, const int32_t* mod_plus,
                                const int32_t* cov_minus, const int32_t* mod_minus, char* out, int64_t cap, int64_t* n_lines) {
    bmk::Name name = {};
    if (!bmk::set_name(name, contig_name)) return fail(DM_EINVAL, "dm_bedmerge_format_host: a contig name of 1 to %d printable bytes", bed::MAX_NAME);
    if (first_pos < 0 || length < 0 || first_pos + length > bmk::MAX_LENGTH || cap < 0)
        return fail(DM_EINVAL, "dm_bedmerge_format_host: positions %lld .. +%lld (inside 0 .. 2^31 - 2)", (long long)first_pos, (long long)length);
    if ((cov_plus == nullptr) != (mod_plus == nullptr) || (cov_minus == nullptr) != (mod_minus == nullptr))
        return fail(DM_EINVAL, "dm_bedmerge_format_host: a strand is given by both of its tables or by neither");
    int64_t bad = -1;
    const int64_t bytes = bmk::format_tables(name, base, first_pos, length, cov_plus, mod_plus, cov_minus, mod_minus, out, cap, n_lines, &bad);
    if (bytes < 0) return fail(DM_EINVAL, "dm_bedmerge_format_host: the sums of position %lld are outside 0 <= modified <= coverage", (long long)(first_pos + bad));
    return bytes;
}

int dm_bedmerge_add_text(dm_bedmerge* h, const char* text, int64_t n_bytes, int64_t* n_lines, int32_t* flag, int64_t* first_bad_line) {
    using B = dm_bedmerge;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (n_lines) *n_lines = 0;
    if (flag) *flag = 0;
    if (first_bad_line) *first_bad_line = -1;
    if (!h->plus) return fail(DM_ESTATE, "dm_bedmerge_add_text: no contig");
    h->n_records = 0;
    HIP_TRY(hipSetDevice(h->xy->device));
    hipStream_t s = h->xy->stream;
    unsigned long long* d_stat = h->b.ptr<unsigned long long>(B::STAT);
    if (n_bytes > 0) HIP_TRY(hipMemsetAsync(d_stat, 0, bmk::N_STAT * 8, s));
    int rc;
    long long rows = 0;
    if ((rc = xlk::split(h->xy, h->b, text, n_bytes, bmk::MAX_RECORDS, "dm_bedmerge_add_text", "lines", h->ev[0], &rows)) != DM_OK || rows == 0) return rc;
    if ((rc = bmk::record_buffers(h, rows)) != DM_OK) return rc;
    const long long limit = h->fixed ? (long long)dm_summary_length(h->plus) : bmk::MAX_LENGTH;
    hipLaunchKernelGGL(bmk::bm_parse_kernel, dim3(unsigned((rows + bmk::THREADS - 1) / bmk::THREADS)), dim3(bmk::THREADS), 0, s, h->b.ptr<const char>(xlk::TEXT),
                       h->b.ptr<const long long>(xlk::START), rows, h->name, limit, h->b.ptr<int>(B::POS), h->b.ptr<int>(B::COV), h->b.ptr<int>(B::MOD),
                       h->b.ptr<unsigned char>(B::STRAND), h->b.ptr<unsigned char>(xlk::STATUS), d_stat);
    HIP_TRY(hipGetLastError());
    if ((rc = xlk::first_bad(h->xy, h->b, rows)) != DM_OK) return rc;
    HIP_TRY(hipEventRecord(h->ev[1], s));
    long long first = -1;
    unsigned long long stat[bmk::N_STAT] = {};
    HIP_TRY(hipMemcpyAsync(&first, h->b.buf[xlk::OUT], 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = add_time(h->ev[0], h->ev[1], h->parse_ms)) != DM_OK) return rc;
    if (n_lines) *n_lines = rows;
    if (first >= 0) {                                                // outside the grammar: nothing of this text is added
        if (flag) *flag = 1;
        if (first_bad_line) *first_bad_line = first + 1;
        return DM_OK;
    }
    h->n_records = rows;
    return bmk::add_device_records(h, rows, int64_t(stat[bmk::S_MAXPOS]), int64_t(stat[bmk::S_MAXCOV]));
}

int dm_bedmerge_add_records(dm_bedmerge* h, int64_t n, const int32_t* pos, const uint8_t* strand, const int32_t* cov, const int32_t* mod) {
    using B = dm_bedmerge;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!h->plus) return fail(DM_ESTATE, "dm_bedmerge_add_records: no contig");
    if (n < 0 || n > bmk::MAX_RECORDS || (n > 0 && (!pos || !strand || !cov || !mod))) return fail(DM_EINVAL, "dm_bedmerge_add_records: %lld records", (long long)n);
    const int64_t limit = h->fixed ? dm_summary_length(h->plus) : int64_t(bmk::MAX_LENGTH);
    int64_t max_pos = 0, max_cov = 0;
    for (int64_t i = 0; i < n; ++i) {                                // what the kernel indexes with, checked before any launch
        if (pos[i] < 0 || pos[i] >= limit || strand[i] > 1 || cov[i] < 0 || mod[i] < 0 || mod[i] > cov[i])
            return fail(DM_EINVAL, "dm_bedmerge_add_records: record %lld (position %d of %lld, strand %d, coverage %d, modified %d)", (long long)i, pos[i], (long long)limit,
                        int(strand[i]), cov[i], mod[i]);
        max_pos = std::max<int64_t>(max_pos, pos[i]);
        max_cov = std::max<int64_t>(max_cov, cov[i]);
    }
    h->n_records = 0;
    if (n == 0) return DM_OK;
    HIP_TRY(hipSetDevice(h->xy->device));
    int rc = bmk::record_buffers(h, n);
    if (rc) return rc;
    hipStream_t s = h->xy->stream;
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::POS], pos, size_t(n) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::COV], cov, size_t(n) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::MOD], mod, size_t(n) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::STRAND], strand, size_t(n), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->n_records = n;
    return bmk::add_device_records(h, n, max_pos, max_cov);
}

int dm_bedmerge_fetch_records(dm_bedmerge* h, int32_t* pos, uint8_t* strand, int32_t* cov, int32_t* mod) {
    using B = dm_bedmerge;
    if (!h) return fail(DM_EINVAL, "null handle");
    const size_t n = size_t(h->n_records);
    if (n == 0) return DM_OK;
    HIP_TRY(hipSetDevice(h->xy->device));
    if (pos) HIP_TRY(hipMemcpy(pos, h->b.buf[B::POS], n * 4, hipMemcpyDeviceToHost));
    if (cov) HIP_TRY(hipMemcpy(cov, h->b.buf[B::COV], n * 4, hipMemcpyDeviceToHost));
    if (mod) HIP_TRY(hipMemcpy(mod, h->b.buf[B::MOD], n * 4, hipMemcpyDeviceToHost));
    if (strand) HIP_TRY(hipMemcpy(strand, h->b.buf[B::STRAND], n, hipMemcpyDeviceToHost));
    return DM_OK;
}

int dm_bedmerge_format_begin(dm_bedmerge* h, char base, int64_t* n_lines, int64_t* n_bytes, int64_t* largest_tile_bytes) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->text.clear();
    if (n_lines) *n_lines = 0;
    if (n_bytes) *n_bytes = 0;
    if (largest_tile_bytes) *largest_tile_bytes = 0;
    if (!h->plus) return fail(DM_ESTATE, "dm_bedmerge_format_begin: no contig");
    if ((unsigned char)base < 0x21 || (unsigned char)base > 0x7e) return fail(DM_EINVAL, "dm_bedmerge_format_begin: base byte %d", int(base));
    HIP_TRY(hipSetDevice(h->xy->device));
    int rc;
    if ((rc = dm_summary_sync(h->plus)) != DM_OK || (rc = dm_summary_sync(h->minus)) != DM_OK) return rc;
    const int64_t length = dm_summary_length(h->plus);
    if (length != dm_summary_length(h->minus) || length < 1 || length > bmk::MAX_LENGTH)
        return fail(DM_ESTATE, "dm_bedmerge_format_begin: tables of %lld and %lld positions", (long long)length, (long long)dm_summary_length(h->minus));
    HIP_TRY(hipMemsetAsync(h->b.ptr<unsigned long long>(dm_bedmerge::STAT) + bmk::S_BADSUM, 0, 8, h->xy->stream));
    txo::Totals t;
    if ((rc = h->text.begin(h->xy, bmk::emitter(h, base, length), length, "dm_bedmerge_format_begin", t)) != DM_OK) return rc;
    if (t.bad_tiles) {
        h->text.clear();
        return fail(DM_EINVAL, "dm_bedmerge_format_begin: the sums of %llu tiles left 0 <= modified <= coverage (int32 overflow through repeated keys)", t.bad_tiles);
    }
    h->format_length = length;
    h->format_base = base;
    if (n_lines) *n_lines = t.lines;
    if (n_bytes) *n_bytes = t.bytes;
    if (largest_tile_bytes) *largest_tile_bytes = t.largest_tile;
    return DM_OK;
}

// -> 1: text was returned and more follows, 0: this was the last run (or there is no text), < 0: an error
int dm_bedmerge_format_next(dm_bedmerge* h, char* out, int64_t cap, int64_t* got) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (got) *got = 0;
    if (!h->text.begun() || !h->plus) return fail(DM_ESTATE, "dm_bedmerge_format_next: no format begun (or the tables changed since)");
    if (dm_summary_length(h->plus) != h->format_length || dm_summary_length(h->minus) != h->format_length)
        return fail(DM_ESTATE, "dm_bedmerge_format_next: the tables changed since format_begin");
    return h->text.next(h->xy, bmk::emitter(h, h->format_base, h->format_length), h->format_length, "dm_bedmerge_format_next", out, cap, got);
}

int dm_bedmerge_times(dm_bedmerge* h, double* parse_ms, double* add_ms, double* format_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (parse_ms) *parse_ms = h->parse_ms;
    if (add_ms) *add_ms = h->add_ms;
    if (format_ms) *format_ms = h->text.ms;
    return DM_OK;
}

}  // extern "C"
