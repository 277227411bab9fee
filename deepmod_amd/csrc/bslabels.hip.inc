// bslabels.hip.inc — `bslabels`, device part (part of offline.hip): 1 - 4 bisulfite bedMethyl replicates and the reference -> the three position
// lists getfeatures --motifORPos 2 reads (fulmod, anymod, nomod; readPosFiles, myGetFeatureBasedPos.py:672-698).
//   the replicates    bsk::Truth of bsperf.hip.inc: bs_parse_kernel, bs_compact_kernel, bs_fill_kernel - the one copy dm_bsperf runs, with its
//                     grammar, its line classes and its duplicate check; one 32-bit slot per (replicate, strand, position) of the open contig
//   the motif         spk::sp_code_kernel of siteperf.hip.inc on the contig's bytes: one code byte per position, bit 0 '+' site, bit 1 '-' site
//   the classes       bl_class_kernel    one sweep over (strand, position): the R slots and the code byte -> one class byte per key
//                                        (blk::class_of, bslabels.inc); the counters of either strand reduced per wave and per block, one 64-bit atomic per block
//   a list's text     the tiled writer of textout.hip.inc (txo::Run) on blk::Emitter: the lines of a position from the class bytes of its two keys
// deepmod_amd/bslabels.py (HostEngine) is the numpy twin and the statement of the semantics.
// Memory of the open contig: 8 R bytes of slots, 1 byte of reference, 1 code byte and 2 class bytes per position.  The sweep reads 8 R + 1 and
// writes 2 bytes per position; lane i of a wave reads slot i of a replicate's row (the replicate / strand-major table of bs_fill_kernel), so every
// load of a wave is one run of 256 bytes, and the loop over the replicates is inside the lane.
// Exactness and determinism.  A class is a function of the slots and the code byte alone; the counters are integers summed with atomics, and
// integer additions commute.  The format has no atomics: a line's offset is its tile's scanned offset + the block scan of the bytes of the lanes
// before it, and every output byte has one writer.  Two runs give identical bytes.
#pragma once
#include "host.h"
#include "blockscan.hip.inc"
#include "xyrows.hip.inc"
#include "siteperf.hip.inc"
#include "bsperf.hip.inc"
#include "textout.hip.inc"
#include "bslabels.inc"

namespace blk {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;                    // grid of the sweep: a block loops over its share and flushes once

// truth [R][2 strands][length], code [length] -> cls [2 strands][length], counts [2 strands][N_COUNT] +=
__global__ __launch_bounds__(THREADS) void bl_class_kernel(const unsigned* __restrict__ truth, const unsigned char* __restrict__ code, const long long length, const Rule p,
                                                          unsigned char* __restrict__ cls, unsigned long long* __restrict__ counts) {
    long long n[2][N_COUNT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < N_COUNT; ++k) n[s][k] = 0;
    for (long long e = (long long)blockIdx.x * THREADS + threadIdx.x; e < 2 * length; e += (long long)gridDim.x * THREADS) {
        const int s = e >= length ? 1 : 0;
        const long long q = e - (long long)s * length;
        const bool admissible = ((code[q] >> s) & 1u) != 0;
        const int c = class_of(truth + e, 2 * length, p, admissible);            // slot of replicate r: truth[(r * 2 + s) * length + q]
        cls[e] = (unsigned char)c;
        const int k = c == C_NONE ? (admissible ? int(N_BARE) : -1) : c - 1;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < N_COUNT; ++j) n[t][j] += (t == s && j == k) ? 1 : 0;
    }
    // per wave in registers, across the block's waves in LDS, then one 64-bit atomic per block and counter that has something to add.  Ten addresses
    // take every atomic of the sweep: with one atomic per wave and counter (bsk::wave_add) the sweep of 5,000,002 positions took 0.63 ms, with
    // one per block 0.055 ms (profiles/bslabels/README.md)
    __shared__ long long part[THREADS / 64][2 * N_COUNT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < N_COUNT; ++k) {
            long long v = n[s][k];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][s * N_COUNT + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < 2 * N_COUNT) {
        long long v = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) v += part[w][threadIdx.x];
        if (v != 0) atomicAdd(counts + threadIdx.x, (unsigned long long)v);
    }
}

}  // namespace blk

struct dm_bslabels : bsk::Truth {
    hipEvent_t cev[2] = {nullptr, nullptr};             // class: begin / end
    enum { SEQ, CODE, CLS, COUNTS, N_OWN };
    DevBufs<N_OWN> c{"dm_bslabels"};                    // what the classes need on top of the truth side
    blk::Rule rule = {};
    bool classified = false;
    txo::Run text;                                      // the format in progress, of list format_list
    int format_list = 0;
    double class_ms = 0.0;
};

namespace blk {

// the lines of list `list` of the classified contig; false: its name is none a line can hold
bool emitter(const dm_bslabels* h, const int list, Emitter& em) {
    const unsigned char* cls = h->c.ptr<const unsigned char>(dm_bslabels::CLS);
    em.list = list;
    em.cls_p = cls;
    em.cls_m = cls + h->length;
    return blk::set_name(em.name, h->names.s[h->contig]);
}

}  // namespace blk

extern "C" {

int dm_bslabels_tile_positions(void) { return txo::TILE_POS; }

void dm_bslabels_destroy(dm_bslabels* h) {
    if (!h) return;
    bsk::truth_release(h);                                           // (the device is set and the stream drained first)
    h->c.release();
    h->text.release();
    for (hipEvent_t e : h->cev)
        if (e) (void)hipEventDestroy(e);
    delete h;
}

dm_bslabels* dm_bslabels_create(int device, int n_contigs, const char* const* names, const int64_t* lengths, int n_replicates, int cov, int methylated, int unmethylated) {
    if (n_replicates < 1 || n_replicates > bsk::MAX_REP) {
        fail(DM_EINVAL, "dm_bslabels_create: %d replicates (1 to %d)", n_replicates, bsk::MAX_REP);
        return nullptr;
    }
    if (cov < 1 || cov > bsk::MAX_COV) {
        fail(DM_EINVAL, "dm_bslabels_create: a least coverage of %d (1 to %d: a record's coverage saturates there)", cov, bsk::MAX_COV);
        return nullptr;
    }
    if (unmethylated < 0 || methylated > 100 || unmethylated >= methylated) {
        fail(DM_EINVAL, "dm_bslabels_create: 0 <= unmethylated < methylated <= 100 (got %d, %d)", unmethylated, methylated);
        return nullptr;
    }
    bsk::Names nm;
    int which = bsk::set_names(nm, n_contigs, names, lengths);
    for (int k = 0; !which && k < n_contigs; ++k)
        if (!lengths || lengths[k] < 1) which = k + 1;                // the lists are for getfeatures, which refuses a position outside the reference
    if (which) {
        fail(DM_EINVAL, "dm_bslabels_create: 1 to %d distinct contig names of 1 to %d printable bytes, every length known, 1 to 2^31 - 1 (contig %d of %d)", bsk::MAX_CONTIGS,
             bsk::MAX_NAME, which - 1, n_contigs);
        return nullptr;
    }
    dm_bslabels* h = new dm_bslabels;
    h->rule = {n_replicates, cov, methylated, unmethylated};
    if (!bsk::truth_init(h, device, nm, n_replicates, "dm_bslabels", "dm_bslabels_create")) {
        dm_bslabels_destroy(h);
        return nullptr;
    }
    bool ok = h->text.init("dm_bslabels");
    for (hipEvent_t& e : h->cev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && h->c.ensure(dm_bslabels::COUNTS, 2 * blk::N_COUNT * 8) == DM_OK;
    if (!ok) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_bslabels_create: events or counters on device %d", device);
        dm_bslabels_destroy(h);
        return nullptr;
    }
    return h;
}

int dm_bslabels_add_truth_text(dm_bslabels* h, int replicate, const char* text, int64_t n_bytes, int is_first_chunk, int64_t* lines, int64_t* n_records, int32_t* flag,
                               int64_t* first_bad_line) {
    if (!h) return fail(DM_EINVAL, "null handle");
    return bsk::truth_add_text(h, "dm_bslabels_add_truth_text", replicate, text, n_bytes, is_first_chunk, lines, n_records, flag, first_bad_line);
}

int dm_bslabels_add_truth_records(dm_bslabels* h, int replicate, int64_t n, const uint8_t* contig, const uint8_t* strand, const int32_t* pos, const int32_t* cov,
                                  const int32_t* pct, const int64_t* lines) {
    if (!h) return fail(DM_EINVAL, "null handle");
    return bsk::truth_add_records(h, "dm_bslabels_add_truth_records", replicate, n, contig, strand, pos, cov, pct, lines);
}

int dm_bslabels_fetch_records(dm_bslabels* h, int32_t* pos, uint32_t* meta) {
    if (!h) return fail(DM_EINVAL, "null handle");
    return bsk::truth_fetch_records(h, pos, meta);
}

int dm_bslabels_close_contig(dm_bslabels* h) {
    if (!h) return fail(DM_EINVAL, "null handle");
    bsk::truth_close(h);
    h->classified = false;
    h->text.clear();
    return DM_OK;
}

int dm_bslabels_open(dm_bslabels* h, int contig_index, const uint8_t* seq, int64_t len, const char* motif, int m, int k) {
    using B = dm_bslabels;
    if (!h) return fail(DM_EINVAL, "null handle");
    (void)dm_bslabels_close_contig(h);
    if (contig_index < 0 || contig_index >= h->names.n) return fail(DM_EINVAL, "dm_bslabels_open: contig %d of %d", contig_index, h->names.n);
    if (!seq || len != h->names.limit[contig_index])
        return fail(DM_EINVAL, "dm_bslabels_open: %lld reference bytes for a contig of %lld positions", (long long)len, (long long)h->names.limit[contig_index]);
    if (!motif || m < 1 || m > blk::MAX_MOTIF || k < 0 || k >= m)
        return fail(DM_EINVAL, "dm_bslabels_open: motif of %d bases (1 to %d), modified offset %d", m, blk::MAX_MOTIF, k);
    spk::Motif mo = {};
    const int other = spk::make_motif(mo, motif, m, k);
    if (other >= 0) return fail(DM_EINVAL, "dm_bslabels_open: motif base %d is none of A, C, G, T", other);
    HIP_TRY(hipSetDevice(h->xy->device));
    // what the contig needs that the handle does not hold yet, as DevBufs would allocate it, against what is free: refused before any launch
    const size_t want[4] = {size_t(h->n_rep) * 2 * size_t(len) * 4, size_t(len), size_t(len), size_t(len) * 2};
    const size_t held[4] = {h->b.cap[bsk::Truth::TRUTH], h->c.cap[B::SEQ], h->c.cap[B::CODE], h->c.cap[B::CLS]};
    size_t need = 0, total = 0, free_bytes = 0, all_bytes = 0;
    for (int j = 0; j < 4; ++j) {
        total += want[j];
        if (held[j] < want[j]) need += want[j] + (want[j] >> 2) + 256;
    }
    HIP_TRY(hipMemGetInfo(&free_bytes, &all_bytes));
    size_t freed = 0;
    for (int j = 0; j < 4; ++j)
        if (held[j] < want[j]) freed += held[j];
    if (need > free_bytes + freed)
        return fail(DM_ENOMEM, "dm_bslabels_open: contig %d of %lld positions and %d replicates needs %zu bytes on the device (%zu to allocate, %zu are free)", contig_index,
                    (long long)len, h->n_rep, total, need, free_bytes + freed);
    int rc;
    if ((rc = h->c.ensure(B::SEQ, size_t(len))) != DM_OK || (rc = h->c.ensure(B::CODE, size_t(len))) != DM_OK || (rc = h->c.ensure(B::CLS, size_t(len) * 2)) != DM_OK) return rc;
    // the site codes first: the contig is open only once they and the zeroed slots are there
    hipStream_t s = h->xy->stream;
    HIP_TRY(hipMemcpyAsync(h->c.buf[B::SEQ], seq, size_t(len), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(h->cev[0], s));
    hipLaunchKernelGGL(spk::sp_code_kernel, dim3(unsigned((len + spk::THREADS - 1) / spk::THREADS)), dim3(spk::THREADS), 0, s, h->c.ptr<const unsigned char>(B::SEQ),
                       (long long)len, mo, 0ll, (long long)(len - 1), h->c.ptr<unsigned char>(B::CODE));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->cev[1], s));
    HIP_TRY(hipStreamSynchronize(s));                                // the caller's bytes are read by now
    if ((rc = add_time(h->cev[0], h->cev[1], h->fill_ms)) != DM_OK) return rc;       // preparing the contig's tables: with the fill
    if ((rc = bsk::truth_open(h, contig_index, len)) != DM_OK) bsk::truth_close(h);
    return rc;
}

int dm_bslabels_fill(dm_bslabels* h, int replicate, int64_t n, const int32_t* pos, const uint32_t* meta, int64_t* dup_pos, int32_t* dup_strand) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (dup_pos) *dup_pos = -1;
    if (dup_strand) *dup_strand = -1;
    if (h->contig < 0) return fail(DM_ESTATE, "dm_bslabels_fill: no contig");
    if (h->classified) return fail(DM_ESTATE, "dm_bslabels_fill: the contig has been classified");
    return bsk::truth_fill(h, "dm_bslabels_fill", replicate, n, pos, meta, dup_pos, dup_strand);
}

int dm_bslabels_classify(dm_bslabels* h, int64_t* counts) {
    using B = dm_bslabels;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!counts) return fail(DM_EINVAL, "dm_bslabels_classify: null argument");
    if (h->contig < 0) return fail(DM_EINVAL, "dm_bslabels_classify: no contig is open");
    if (h->refused) return fail(DM_ESTATE, "dm_bslabels_classify: the contig was refused for a key that occurs twice in a replicate");
    if (h->classified) return fail(DM_EINVAL, "dm_bslabels_classify: the contig has been classified (once per open)");
    HIP_TRY(hipSetDevice(h->xy->device));
    hipStream_t s = h->xy->stream;
    unsigned long long* d_counts = h->c.ptr<unsigned long long>(B::COUNTS);
    const dim3 grid{unsigned(std::min<int64_t>((2 * h->length + blk::THREADS - 1) / blk::THREADS, blk::MAX_BLOCKS))};
    HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * blk::N_COUNT * 8, s));
    HIP_TRY(hipEventRecord(h->cev[0], s));
    hipLaunchKernelGGL(blk::bl_class_kernel, grid, dim3(blk::THREADS), 0, s, h->b.ptr<const unsigned>(bsk::Truth::TRUTH), h->c.ptr<const unsigned char>(B::CODE),
                       (long long)h->length, h->rule, h->c.ptr<unsigned char>(B::CLS), d_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->cev[1], s));
    long long got[2 * blk::N_COUNT] = {};
    HIP_TRY(hipMemcpyAsync(got, d_counts, sizeof got, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int rc;
    if ((rc = add_time(h->cev[0], h->cev[1], h->class_ms)) != DM_OK) return rc;
    for (int j = 0; j < 2 * blk::N_COUNT; ++j) counts[j] = got[j];
    h->classified = true;
    return DM_OK;
}

int dm_bslabels_fetch_classes(dm_bslabels* h, uint8_t* cls) {
    if (!h || !cls) return fail(DM_EINVAL, "null argument");
    if (h->contig < 0 || !h->classified) return fail(DM_ESTATE, "dm_bslabels_fetch_classes: no classified contig");
    HIP_TRY(hipSetDevice(h->xy->device));
    HIP_TRY(hipMemcpy(cls, h->c.buf[dm_bslabels::CLS], size_t(h->length) * 2, hipMemcpyDeviceToHost));
    return DM_OK;
}

int64_t dm_bslabels_format_host(const char* name, int list, const uint8_t* cls_plus, const uint8_t* cls_minus, int64_t first_pos, int64_t length, char* out, int64_t cap) {
    blk::Name nm = {};
    if (!blk::set_name(nm, name)) return fail(DM_EINVAL, "dm_bslabels_format_host: a contig name of 1 to %d printable bytes", bsk::MAX_NAME);
    if (list < blk::C_FUL || list > blk::C_NO) return fail(DM_EINVAL, "dm_bslabels_format_host: list %d (1 fulmod, 2 anymod, 3 nomod)", list);
    if (first_pos < 0 || length < 0 || first_pos + length > blk::MAX_LENGTH || cap < 0)
        return fail(DM_EINVAL, "dm_bslabels_format_host: positions %lld .. +%lld (inside 0 .. 2^31 - 2)", (long long)first_pos, (long long)length);
    return blk::format_classes(nm, list, first_pos, length, cls_plus, cls_minus, out, cap, nullptr);
}

int dm_bslabels_format_begin(dm_bslabels* h, int list, int64_t* n_lines, int64_t* n_bytes, int64_t* largest_tile_bytes) {
    if (!h) return fail(DM_EINVAL, "null handle");
    h->text.clear();
    if (n_lines) *n_lines = 0;
    if (n_bytes) *n_bytes = 0;
    if (largest_tile_bytes) *largest_tile_bytes = 0;
    if (list < blk::C_FUL || list > blk::C_NO) return fail(DM_EINVAL, "dm_bslabels_format_begin: list %d (1 fulmod, 2 anymod, 3 nomod)", list);
    if (h->contig < 0 || !h->classified) return fail(DM_ESTATE, "dm_bslabels_format_begin: no classified contig");
    blk::Emitter em = {};
    if (!blk::emitter(h, list, em)) return fail(DM_ESTATE, "dm_bslabels_format_begin: the name of contig %d", h->contig);
    txo::Totals t;
    const int rc = h->text.begin(h->xy, em, h->length, "dm_bslabels_format_begin", t);
    if (rc != DM_OK) return rc;
    h->format_list = list;
    if (n_lines) *n_lines = t.lines;
    if (n_bytes) *n_bytes = t.bytes;
    if (largest_tile_bytes) *largest_tile_bytes = t.largest_tile;
    return DM_OK;
}

// -> 1: text was returned and more follows, 0: this was the last run (or there is no text), < 0: an error
int dm_bslabels_format_next(dm_bslabels* h, char* out, int64_t cap, int64_t* got) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (got) *got = 0;
    if (!h->text.begun() || h->contig < 0 || !h->classified) return fail(DM_ESTATE, "dm_bslabels_format_next: no format begun");
    blk::Emitter em = {};
    if (!blk::emitter(h, h->format_list, em)) return fail(DM_ESTATE, "dm_bslabels_format_next: the name of contig %d", h->contig);
    return h->text.next(h->xy, em, h->length, "dm_bslabels_format_next", out, cap, got);
}

int dm_bslabels_times(dm_bslabels* h, double* parse_ms, double* fill_ms, double* class_ms, double* format_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (parse_ms) *parse_ms = h->parse_ms;
    if (fill_ms) *fill_ms = h->fill_ms;
    if (class_ms) *class_ms = h->class_ms;
    if (format_ms) *format_ms = h->text.ms;
    return DM_OK;
}

}  // extern "C"
