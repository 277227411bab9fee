// rowsbatch.inc — one worker batch of reads -> the device-ready arrays of the streaming detect (host C++, part of
// feed.hip).
//
// The streaming worker hands the device, per batch: feature rows [R][7] fp32 (the reads' `tx` matrices back to back, 100 zero
// rows of padding on both sides of every read), and per row a reference position and a flag byte, plus "extra" (position, flag)
// pairs for table rows that own no window.  Building them was per-read Python / numpy (15 feeder processes per GPU); here it
// is one pass of compiled code per batch.  Reference semantics, all under /root/reference/bin/DeepMod_scripts/myDetect.py:
//   getEvent (Albacore-2 'simple')              :237-251   dm_events_merge
//   handle_record's filters and alignment walk  :497-713   dm_map_read (readmap.inc) + the checks below
//   get_Feature (fnum = 7)                      :839-903   feature rows of a raw read
//   mPredict1's window / base association       :794-803, :824-833   row k + 100 <-> k-th table row whose readbase is not '-'
//   sum_handler's per-base flags                :1089-1100 flags: bit0 refbase == Base, bit1 readbase != '-'
#pragma once
#include "host.h"

#include <cstdlib>
#include <memory>
#include <mutex>
#include <numeric>

namespace rowsbatch {

enum Status : int64_t {
    OK = 0,
    LESS_EVENT = 1,        // fewer than 50 aligned events (:702-705)
    INDEX_ERROR = 2,       // fewer aligned table rows than aligned events (the reference raises IndexError in mPredict1)
    NO_MATCH = 3,          // no matching base at all (:617-622)
    CIGAR_ERROR = 4,       // malformed CIGAR / runs past read or reference
    FILTERED = 5,          // region filter / caller asked to skip
    NO_REFERENCE = 6,      // contig without a reference sequence
    NOT_MATCHING = 7,      // raw reads: event bases differ from the table's read bases (get_Feature :868-874: the read is dropped)
};
struct BaseCodeTable {         // A, C, G, T -> 0..3 (the one-hot column of get_Feature, myDetect.py:892-896), anything else 255
    unsigned char t[256];
    constexpr BaseCodeTable() : t() {
        for (int i = 0; i < 256; ++i) t[i] = 255;
        t['A'] = 0; t['C'] = 1; t['G'] = 2; t['T'] = 3;
    }
};
constexpr BaseCodeTable kBaseCode{};
constexpr int INFO = 8;    // per-read info: status, contig, strand, windows, rows, table rows, mismatches, extras
constexpr int64_t PAD = 100;

struct Read {
    int64_t status = OK;
    int32_t contig = -1, strand = 0;
    int64_t start_clip = 0, end_clip = 0, n_events = 0, n_al = 0;
    // table: borrowed (packed containers) or, for raw reads, rows [tab_off, tab_off + ntab) of the batch's arena (the pointers are set when the
    // arena has stopped growing: at the end of every dm_rows_add_raw)
    const char* refb = nullptr;
    const char* readb = nullptr;
    const int64_t* refi = nullptr;
    int64_t ntab = 0;
    int64_t tab_off = -1;
    // feature rows: borrowed tx (packed), or built from the event table (raw)
    const float* tx = nullptr;
    int64_t nrows = 0;
    const float* ev_mean = nullptr;      // raw: per event, [n_events]
    const float* ev_stdv = nullptr;
    const float* ev_mean2 = nullptr;     // raw: the signal stage's statistics for events [0, n_stat)
    const float* ev_stdv2 = nullptr;     // (NULL with n_stat > 0: they stay on the device, dm_signal_event_stats_device - the resident form)
    int64_t n_stat = 0;
    int64_t ev_first = 0;                // raw: index of the read's first event in the batch's merged event tables
    const uint64_t* ev_length = nullptr;
    const char* ev_base = nullptr;       // basecalled base of every event
    bool raw = false;
    int64_t mismatches = 0, extras = 0, nsel = 0;       // nsel: windows centred on a base of interest (the only ones whose class reaches the BED)
    int64_t first_bad_row = -1, first_bad_event = -1;
};

}  // namespace rowsbatch

namespace rowsbatch {

// Alignment tables of the raw reads of one batch: three columns that only grow (malloc / realloc: no zero fill, no per-read allocation - a read's
// table used to be three std::vectors of its own, i.e. an mmap, 35 page faults and a munmap per read).  Arenas are kept between batches: a feeder
// process prepares one batch after the other and its tables stay warm.
struct Arena {
    char* refb = nullptr;
    char* readb = nullptr;
    int64_t* refi = nullptr;
    int64_t cap = 0, used = 0;
    bool reserve(int64_t rows) {
        if (rows <= cap) return true;
        const int64_t want = rows + (rows >> 2) + 4096;
        char* a = static_cast<char*>(std::realloc(refb, size_t(want)));
        if (a) refb = a;
        char* b = static_cast<char*>(std::realloc(readb, size_t(want)));
        if (b) readb = b;
        int64_t* c = static_cast<int64_t*>(std::realloc(refi, size_t(want) * sizeof(int64_t)));
        if (c) refi = c;
        if (!a || !b || !c) return false;
        cap = want;
        return true;
    }
    ~Arena() {
        std::free(refb);
        std::free(readb);
        std::free(refi);
    }
};

struct ArenaPool {
    std::mutex mu;
    std::vector<Arena*> idle;
    Arena* take() {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!idle.empty()) {
                Arena* a = idle.back();
                idle.pop_back();
                a->used = 0;
                return a;
            }
        }
        return new (std::nothrow) Arena();
    }
    void give(Arena* a) {
        if (!a) return;
        if (a->cap > (int64_t(1) << 28)) {         // an unusually large batch: do not keep 2.5 GB around for the rest of the run
            delete a;
            return;
        }
        std::lock_guard<std::mutex> lk(mu);
        if (idle.size() < 8) idle.push_back(a);
        else delete a;
    }
    ~ArenaPool() {
        for (Arena* a : idle) delete a;
    }
};
inline ArenaPool& arena_pool() {
    static ArenaPool pool;
    return pool;
}

}  // namespace rowsbatch

struct dm_rowsbatch {
    char base = 'C';
    std::vector<std::unique_ptr<rowsbatch::Read>> reads;
    int64_t n_rows = 0, n_extra = 0, n_sel = 0;
    bool planned = false;
    bool resident = false;               // raw reads whose signal statistics stay on the device (dm_rows_emit_resident)
    rowsbatch::Arena* arena = nullptr;   // tables of the raw reads
    ~dm_rowsbatch() { rowsbatch::arena_pool().give(arena); }
};

namespace rowsbatch {

// counts of a read whose table and clips are known: windows, rows, extras, status (stream.rows_from_packed's rules)
inline void plan_read(Read& r, char base) {
    // clips come from a container's metadata: checked BEFORE any arithmetic with them (clips near INT64_MAX would wrap the
    // subtraction into a plausible n_al and ev_base[start_clip + k] would be read far outside the column)
    // Negative values are an index error of the ledger; clips that are merely too LARGE for the read leave no aligned event - "Less Event",
    // what n_events - start_clip - end_clip < 50 gives in the Python restatement (stream.rows_from_packed) and in the reference (myDetect.py:702-705)
    if (r.start_clip < 0 || r.end_clip < 0 || r.n_events < 0 || r.ntab < 0) {
        r.n_al = 0;
        if (r.status == OK) r.status = INDEX_ERROR;
        return;
    }
    if (r.start_clip > r.n_events || r.end_clip > r.n_events - r.start_clip) {
        r.n_al = 0;
        if (r.status == OK) r.status = LESS_EVENT;
        return;
    }
    r.n_al = r.n_events - r.start_clip - r.end_clip;
    if (r.status != OK) return;
    int64_t n_have = 0;
    for (int64_t j = 0; j < r.ntab; ++j) n_have += r.readb[j] != '-';
    if (r.n_al < 50) {
        r.status = LESS_EVENT;
        return;
    }
    if (n_have < r.n_al || (!r.raw && r.nrows != r.n_al + 2 * PAD)) {
        r.status = INDEX_ERROR;
        return;
    }
    if (r.raw) r.nrows = r.n_al + 2 * PAD;
    // event base vs table base of every aligned row; extras = rows of the wanted base that own no window
    int64_t k = 0, extras = 0, bad = 0, nsel = 0;
    for (int64_t j = 0; j < r.ntab; ++j) {
        const bool not_gap = r.readb[j] != '-';
        const bool sel = not_gap && k < r.n_al;
        if (sel && r.ev_base && r.ev_base[r.start_clip + k] != r.readb[j]) {
            if (!bad) {
                r.first_bad_row = j;
                r.first_bad_event = r.start_clip + k;
            }
            ++bad;
        }
        if (r.refb[j] == base) {
            if (sel) ++nsel;
            else ++extras;
        }
        if (not_gap) ++k;
    }
    r.mismatches = bad;
    r.extras = extras;
    r.nsel = nsel;
    if (bad && r.raw) r.status = NOT_MATCHING;
}

// an offset table of n + 1 entries into an array of `total` elements: starts at >= 0, never decreases, ends inside the array
inline bool offsets_ok(const int64_t* off, int64_t n, int64_t total) {
    if (off[0] < 0) return false;
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return off[n] <= total;
}

// dm_move_events: 0x80 in every byte of the eight at p that equals 1 (exact - no carry crosses a byte), byte j of memory in bits 8 j .. 8 j + 7
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
constexpr bool kMoveWords = true;
#else
constexpr bool kMoveWords = false;
#endif
inline uint64_t move_ones8(const uint8_t* p) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    const uint64_t x = v ^ 0x0101010101010101ull, m = 0x7f7f7f7f7f7f7f7full;
    return ~(((x & m) + m) | x | m);
}

}  // namespace rowsbatch

extern "C" {

// getEvent, Albacore-2 'simple' branch (myDetect.py:237-251), for all reads of a batch: an event starts at index 0 and wherever
// move > 0; stay events (move == 0) are merged into the event before them (lengths added); mean / stdv are the head's, rounded to 3
// decimals like numpy.round (rint(x * 1000) / 1000 in float64) and stored as float32; base = model_state[2].
// model_state: UCS-4 code points, `ms_width` per event (numpy 'U5': 5).  Outputs are sized for the unmerged count.  Returns the
// number of merged events (mev_off[n_reads]) or a negative code.  n_events: entries of the input columns; an ev_off that decreases or
// runs past them (a damaged container) is DM_EINVAL.  m_mean / m_stdv may both be NULL (the values are then not produced, mean / stdv not read).
int64_t dm_events_merge(int64_t n_reads, int64_t n_events, const int64_t* ev_off, const double* mean, const double* stdv, const uint64_t* start,
                        const uint64_t* length, const uint32_t* model_state, int32_t ms_width, const int64_t* move, int64_t* mev_off,
                        float* m_mean, float* m_stdv, uint64_t* m_start, uint64_t* m_length, char* m_base) {
#pragma clang fp contract(off)      // (x * 1000 + M must stay two roundings: see rint_even below)
    // m_mean == m_stdv == NULL (round 6): the rounded basecaller values are not produced - they are read only for events at or behind a read's first
    // empty event (myDetect.py:334-340), which a batch rarely has; a caller that finds one asks again.  16 of the 60 bytes per event and two float64
    // divisions per event are then never touched.
    const bool values = m_mean && m_stdv;
    if (n_reads < 0 || !ev_off || !start || !length || !model_state || !move || !mev_off || (values && (!mean || !stdv)) || (!m_mean != !m_stdv) ||
        !m_start || !m_length || !m_base || ms_width < 3)
        return fail(DM_EINVAL, "dm_events_merge: bad argument");
    if (!rowsbatch::offsets_ok(ev_off, n_reads, n_events))
        return fail(DM_EINVAL, "dm_events_merge: the event offsets decrease or run past the %lld events of the table", (long long)n_events);
    // np.round(x, 3) = rint(x * 1000) / 1000.  rint through the 1.5 * 2^52 constant (round to nearest even in the default rounding mode, the value
    // std::nearbyint returns, for |v| < 2^51): std::nearbyint is a libm CALL in a baseline x86-64 build - two per event were most of this function.
    // (v + M) - M gives +0.0 where numpy gives -0.0 for v in (-0.5, 0): the sign of the input is put back, so the float32 bits are numpy's
    auto rint_even = [](double v) {
        constexpr double M = 6755399441055744.0;
        return std::fabs(v) < 2251799813685248.0 ? std::copysign((v + M) - M, v) : std::nearbyint(v);
    };
    // (outputs through restrict-qualified locals: m_base is a byte pointer, whose stores the compiler must otherwise assume to alias every input)
    float* __restrict o_mean = m_mean;
    float* __restrict o_stdv = m_stdv;
    uint64_t* __restrict o_start = m_start;
    uint64_t* __restrict o_len = m_length;
    char* __restrict o_base = m_base;
    const size_t msw = size_t(ms_width);
    int64_t w = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        mev_off[r] = w;
        const int64_t e0 = ev_off[r], e1 = ev_off[r + 1];
        for (int64_t i = e0; i < e1; ++i) {
            if (i == e0 || move[i] > 0) {
                if (values) {
                    o_mean[w] = float(rint_even(mean[i] * 1000.0) / 1000.0);
                    o_stdv[w] = float(rint_even(stdv[i] * 1000.0) / 1000.0);
                }
                o_start[w] = start[i];
                o_len[w] = length[i];
                const uint32_t cp = model_state[size_t(i) * msw + 2];
                o_base[w] = cp < 128 ? char(cp) : '?';
                ++w;
            } else {
                o_len[w - 1] += length[i];
            }
        }
    }
    mev_off[n_reads] = w;
    return w;
}

// getEvent with --move (myDetect.py:136-153 -> MoveTable.getMove_Info, MoveTable.py:7-54), for all reads of a container: the event table of a read
// from its basecaller MOVE TABLE.  A boundary is every table index i in 1 .. L-1 with move[i] == 1 (move[0] is never looked at, any other value is no
// boundary); the stride is the reference's constant 2 (:30-33).  Event 0 starts at first_sample_template, boundary i ends the current event and starts
// the next at first + 2 i, the last event ends at the read's last sample.  The bases are the Fastq sequence itself.  Where the reference is undefined
// the read FAILS (status, no events written, mev_off[r + 1] == mev_off[r]):
//   DM_MOVE_COUNT     boundaries != bases - 1 (the reference raises IndexError for too many and leaves np.empty rows uninitialised for too few)
//   DM_MOVE_OUTSIDE   first < 0, first >= samples, or the last boundary starts its event at or behind the read's end (np.mean of an empty slice;
//                     a negative length wrapped into uint64)
// so every event of a read that passes is non-empty and inside the signal.  DM_MOVE_COUNT is decided first.  All tables come from disk: offsets are
// checked against n_move / n_fq / the sample offsets' own order before a byte is read; outputs are sized for n_fq events.
// Returns the number of events written (mev_off[n_reads]) or a negative code.
int64_t dm_move_events(int64_t n_reads, int64_t n_move, const uint8_t* move, const int64_t* mv_off, const int64_t* first, const int64_t* raw_off,
                       int64_t n_fq, const char* fq, const int64_t* fq_off, int64_t* mev_off, int32_t* status, uint64_t* m_start, uint64_t* m_length,
                       char* m_base) {
    if (n_reads < 0 || n_move < 0 || n_fq < 0 || !mv_off || !first || !raw_off || !fq_off || !mev_off || !status || (n_move > 0 && !move) ||
        (n_fq > 0 && (!fq || !m_start || !m_length || !m_base)))
        return fail(DM_EINVAL, "dm_move_events: bad argument");
    if (!rowsbatch::offsets_ok(mv_off, n_reads, n_move))
        return fail(DM_EINVAL, "dm_move_events: the move offsets decrease or run past the %lld entries of the table", (long long)n_move);
    if (!rowsbatch::offsets_ok(fq_off, n_reads, n_fq))
        return fail(DM_EINVAL, "dm_move_events: the sequence offsets decrease or run past the %lld bases", (long long)n_fq);
    if (!rowsbatch::offsets_ok(raw_off, n_reads, INT64_MAX))
        return fail(DM_EINVAL, "dm_move_events: the signal offsets decrease");
    int64_t w = 0;
    for (int64_t r = 0; r < n_reads; ++r) {
        mev_off[r] = w;
        const uint8_t* mv = move + mv_off[r];
        const int64_t len = mv_off[r + 1] - mv_off[r], nrow = fq_off[r + 1] - fq_off[r], nsig = raw_off[r + 1] - raw_off[r], f = first[r];
        // (eight table entries per step where the byte order allows it: the byte loop was a third of a feeder's time on a run of move containers)
        int64_t nb = 0, last = 0, i = 1;
        for (; rowsbatch::kMoveWords && i + 8 <= len; i += 8)
            if (const uint64_t hit = rowsbatch::move_ones8(mv + i)) {
                nb += __builtin_popcountll(hit);
                last = i + (63 - __builtin_clzll(hit)) / 8;
            }
        for (; i < len; ++i)
            if (mv[i] == 1) {
                ++nb;
                last = i;
            }
        if (nb != nrow - 1) {
            status[r] = DM_MOVE_COUNT;
            continue;
        }
        if (f < 0 || f >= nsig || (nb > 0 && 2 * last >= nsig - f)) {      // (nsig - f > 0 here: no overflow; last < 2^62 for any table in memory)
            status[r] = DM_MOVE_OUTSIDE;
            continue;
        }
        status[r] = DM_MOVE_OK;
        uint64_t pivot = uint64_t(f);
        int64_t k = w;
        auto boundary = [&](const int64_t at) {
            const uint64_t next = uint64_t(f) + 2 * uint64_t(at);
            m_start[k] = pivot;
            m_length[k] = next - pivot;
            pivot = next;
            ++k;
        };
        for (i = 1; rowsbatch::kMoveWords && i + 8 <= len; i += 8)
            for (uint64_t hit = rowsbatch::move_ones8(mv + i); hit; hit &= hit - 1) boundary(i + __builtin_ctzll(hit) / 8);
        for (; i < len; ++i)
            if (mv[i] == 1) boundary(i);
        m_start[k] = pivot;
        m_length[k] = uint64_t(nsig) - pivot;
        std::memcpy(m_base + w, fq + fq_off[r], size_t(nrow));
        w += nrow;
    }
    mev_off[n_reads] = w;
    return w;
}

dm_rowsbatch* dm_rows_create(char base) {
    dm_rowsbatch* h = new (std::nothrow) dm_rowsbatch();
    if (!h) {
        fail(DM_ENOMEM, "out of host memory");
        return nullptr;
    }
    h->base = base;
    return h;
}

void dm_rows_destroy(dm_rowsbatch* h) { delete h; }

// Reads of a packed feature container (deepmod_amd/predstore.py format 2: the arguments the reference hands to mPredict1 at
// myDetect.py:715, all reads back to back).  The arrays are BORROWED until dm_rows_emit / dm_rows_destroy.
// n_tx_rows / n_table_rows / n_events: rows of tx, entries of the three table columns, entries of evbase; n_contigs: contig[i] must be
// in [0, n_contigs).  Offsets that decrease or run past their arrays, a strand other than 0 / 1 or a contig outside the range are
// DM_EINVAL for the whole container (nothing of it is added): a damaged file must not become an out-of-bounds read.
int dm_rows_add_packed(dm_rowsbatch* h, int64_t n_reads, int64_t n_tx_rows, int64_t n_table_rows, int64_t n_events, int32_t n_contigs,
                       const int64_t* row_off, const int64_t* bmi_off, const int64_t* ev_off,
                       const float* tx, const char* refbase, const char* readbase, const int64_t* refbasei, const char* evbase,
                       const int64_t* start_clip, const int64_t* end_clip, const int32_t* contig, const int32_t* strand) {
    if (!h || n_reads < 0 || !row_off || !bmi_off || !ev_off || !refbase || !readbase || !refbasei || !start_clip || !end_clip || !contig || !strand)
        return fail(DM_EINVAL, "dm_rows_add_packed: bad argument");
    if (h->planned) return fail(DM_ESTATE, "dm_rows_add_packed after dm_rows_info");
    if (!rowsbatch::offsets_ok(row_off, n_reads, n_tx_rows) || !rowsbatch::offsets_ok(bmi_off, n_reads, n_table_rows) ||
        !rowsbatch::offsets_ok(ev_off, n_reads, n_events))
        return fail(DM_EINVAL, "dm_rows_add_packed: an offset table decreases or runs past its array (%lld feature rows, %lld table rows, %lld events)",
                    (long long)n_tx_rows, (long long)n_table_rows, (long long)n_events);
    for (int64_t i = 0; i < n_reads; ++i)
        if (contig[i] < 0 || contig[i] >= n_contigs || (strand[i] != 0 && strand[i] != 1))
            return fail(DM_EINVAL, "dm_rows_add_packed: read %lld has contig %d of %d, strand %d", (long long)i, contig[i], n_contigs, strand[i]);
    for (int64_t i = 0; i < n_reads; ++i) {
        auto r = std::make_unique<rowsbatch::Read>();
        r->contig = contig[i];
        r->strand = strand[i];
        r->start_clip = start_clip[i];
        r->end_clip = end_clip[i];
        r->n_events = ev_off[i + 1] - ev_off[i];
        r->refb = refbase + bmi_off[i];
        r->readb = readbase + bmi_off[i];
        r->refi = refbasei + bmi_off[i];
        r->ntab = bmi_off[i + 1] - bmi_off[i];
        r->tx = tx ? tx + row_off[i] * DM_NFEAT : nullptr;
        r->nrows = row_off[i + 1] - row_off[i];
        r->ev_base = evbase ? evbase + ev_off[i] : nullptr;
        if (!tx) r->status = rowsbatch::INDEX_ERROR;
        h->reads.push_back(std::move(r));
    }
    return DM_OK;
}

// Raw reads: one alignment record per read (fields of its SAM line), the merged event tables of the batch (dm_events_merge) with the
// signal stage's statistics (dm_signal_event_stats_batch: s_mean / s_stdv / first_empty; an event before first_empty takes them, the
// ones behind keep the basecaller's; a first empty event beyond index 500 truncates the table to [0, first_empty - 1), :337-340), and
// the reference sequences.  ev_read[i]: which read of the event tables (n_event_reads of them: mev_off has n_event_reads + 1 entries)
// record i belongs to; contig[i] < 0: no reference sequence.
// skip[i] != 0: dropped by the caller (ConUnk).  Region filter = the reference's --region list (:544-553): a record passes if some
// entry has (contig < 0 or == its contig) and (lo < 0 or pos > lo) and (hi < 0 or pos + events < hi); n_region == 0: everything passes.
// The alignment walk and its tables are computed and OWNED here; the event arrays and sequences are BORROWED until emit.
int dm_rows_add_raw(dm_rowsbatch* h, int64_t n_reads, const int32_t* flag, const int64_t* pos1, const char* const* cigar,
                    const char* const* readseq, const int64_t* readseq_len, const int32_t* contig, const int32_t* ev_read,
                    const uint8_t* skip, int32_t n_contigs, const char* const* refseq, const int64_t* refseq_len,
                    int64_t n_event_reads, int64_t n_events, const int64_t* mev_off, const float* m_mean, const float* m_stdv, const uint64_t* m_length, const char* m_base,
                    const float* s_mean, const float* s_stdv, const int64_t* first_empty, int32_t n_region,
                    const int32_t* region_contig, const int64_t* region_lo, const int64_t* region_hi) {
    using namespace rowsbatch;
    if (!h || n_reads < 0 || !flag || !pos1 || !cigar || !readseq || !readseq_len || !contig || !ev_read || !mev_off || (!m_mean != !m_stdv) ||
        !m_length || !m_base || (n_contigs > 0 && (!refseq || !refseq_len)) || (n_region > 0 && (!region_contig || !region_lo || !region_hi)))
        return fail(DM_EINVAL, "dm_rows_add_raw: bad argument");
    // m_mean == m_stdv == NULL: the caller has not produced the basecaller's values (dm_events_merge without them) - fine as long as no read needs them,
    // i.e. every event of every read takes the signal stage's statistics (checked per read below)
    const bool have_fallback = m_mean && m_stdv;
    if (h->planned) return fail(DM_ESTATE, "dm_rows_add_raw after dm_rows_info");
    if (n_event_reads < 0 || !rowsbatch::offsets_ok(mev_off, n_event_reads, n_events))
        return fail(DM_EINVAL, "dm_rows_add_raw: the event offsets decrease or run past the %lld merged events", (long long)n_events);
    for (int64_t i = 0; i < n_reads; ++i)
        if (ev_read[i] < 0 || ev_read[i] >= n_event_reads || !cigar[i] || !readseq[i])
            return fail(DM_EINVAL, "dm_rows_add_raw: record %lld names event table %d of %lld (or has no CIGAR / sequence)", (long long)i, ev_read[i],
                        (long long)n_event_reads);
    auto region_ok = [&](int32_t c, bool with_pos, int64_t pos, int64_t nev) {
        if (n_region <= 0) return true;
        for (int32_t k = 0; k < n_region; ++k) {
            if (!(region_contig[k] < 0 || region_contig[k] == c)) continue;
            if (!with_pos) return true;
            if ((region_lo[k] < 0 || pos > region_lo[k]) && (region_hi[k] < 0 || pos + nev < region_hi[k])) return true;
        }
        return false;
    };
    // statistics on the device (round 6): s_mean == s_stdv == NULL with first_empty given - dm_signal_event_stats_device keeps mean / stdv of every event
    // of the batch in device memory (index = position in the merged tables), first_empty still cuts the tables here, and the batch is written with
    // dm_rows_emit_resident
    const bool resident = !s_mean && !s_stdv && first_empty;
    if (resident) h->resident = true;
    if (!h->arena) h->arena = arena_pool().take();
    if (!h->arena) return fail(DM_ENOMEM, "out of host memory");
    Arena& A = *h->arena;
    const size_t first_new = h->reads.size();
    std::vector<int64_t> caps(size_t(n_reads), 0);
    for (int64_t i = 0; i < n_reads; ++i) {
        auto r = std::make_unique<Read>();
        r->raw = true;
        r->contig = contig[i];
        const int64_t e0 = mev_off[ev_read[i]], e1 = mev_off[ev_read[i] + 1];
        int64_t nev = e1 - e0, nstat = 0;
        if ((s_mean && s_stdv) || resident) {
            nstat = nev;
            if (first_empty) {
                const int64_t fe = first_empty[ev_read[i]];
                if (fe < nev) {
                    nstat = fe < 0 ? 0 : fe;
                    if (fe > 500) nev = fe - 1;          // m_event = ev[:i - 1]
                }
            }
            if (nstat > nev) nstat = nev;
        }
        if (!have_fallback && nstat < nev)
            return fail(DM_EINVAL, "dm_rows_add_raw: record %lld has events without signal statistics (%lld of %lld) and the call has no basecaller values for them",
                        (long long)i, (long long)nstat, (long long)nev);
        r->n_events = nev;
        r->ev_first = e0;
        r->ev_mean = have_fallback ? m_mean + e0 : nullptr;
        r->ev_stdv = have_fallback ? m_stdv + e0 : nullptr;
        r->ev_mean2 = s_mean ? s_mean + e0 : nullptr;
        r->ev_stdv2 = s_stdv ? s_stdv + e0 : nullptr;
        r->n_stat = nstat;
        r->ev_length = m_length + e0;
        r->ev_base = m_base + e0;
        if (skip && skip[i]) r->status = FILTERED;
        else if (!region_ok(r->contig, false, 0, 0)) r->status = FILTERED;
        else if (r->contig < 0 || r->contig >= n_contigs || !refseq[r->contig]) r->status = NO_REFERENCE;
        if (r->status == OK) {
            // rows of the table <= sum of all CIGAR counts, and every row consumes a read base or a reference base
            int64_t cap = 0, cur = 0;
            const int64_t most = (readseq_len[i] > 0 ? readseq_len[i] : 0) + refseq_len[r->contig];
            for (const char* p = cigar[i]; *p; ++p) {
                if (*p >= '0' && *p <= '9') cur = cur > most ? cur : cur * 10 + (*p - '0');
                else {
                    cap = cap + cur > most ? most : cap + cur;
                    cur = 0;
                }
            }
            caps[size_t(i)] = cap + 8;
        }
        h->reads.push_back(std::move(r));
    }
    {
        int64_t need = A.used;
        for (int64_t c : caps) need += c;
        if (!A.reserve(need)) return fail(DM_ENOMEM, "out of host memory (%lld table rows)", (long long)need);
    }
    for (int64_t i = 0; i < n_reads; ++i) {
        Read* r = h->reads[first_new + size_t(i)].get();
        if (r->status != OK) continue;
        int64_t info[DM_MAP_INFO_LEN], first = 0, need = 0;
        const int rc = readmap::map_read_core(flag[i], pos1[i], cigar[i], readseq[i], readseq_len[i], refseq[r->contig], refseq_len[r->contig], r->n_events,
                                              A.refb + A.used, A.readb + A.used, A.refi + A.used, nullptr, caps[size_t(i)], info, &first, &need);
        if (rc != DM_OK || info[DM_MAP_STATUS] == DM_MAP_NEED_ROWS) r->status = CIGAR_ERROR;
        else if (!region_ok(r->contig, true, info[DM_MAP_POS_AFTER_CLIP], info[DM_MAP_EVENTS_AFTER_CLIP])) r->status = FILTERED;
        else if (info[DM_MAP_STATUS] == DM_MAP_NO_MATCH) r->status = NO_MATCH;
        else {
            r->strand = int32_t(info[DM_MAP_STRAND]);
            r->start_clip = info[DM_MAP_LEFTCLIP];
            r->end_clip = info[DM_MAP_RIGHTCLIP];
            r->ntab = info[DM_MAP_N_ROWS];
            r->tab_off = A.used + first;
            if (info[DM_MAP_EV_HI] - info[DM_MAP_EV_LO] < 50) r->status = LESS_EVENT;
            A.used += first + r->ntab;           // (a read that is dropped below keeps its rows: plan_read's counts are what the ledger reports)
        }
    }
    // the arena has stopped growing (until the next call): table pointers of every raw read of the handle
    for (auto& rp : h->reads)
        if (rp->tab_off >= 0) {
            rp->refb = A.refb + rp->tab_off;
            rp->readb = A.readb + rp->tab_off;
            rp->refi = A.refi + rp->tab_off;
        }
    return DM_OK;
}

// Reads whose alignment table the caller already has (its own aligner post-processing, or dm_map_read called per read): the table
// columns of all reads back to back (bmi_off), clips, strand, contig, and the event tables as for dm_rows_add_raw (mev_off indexed by
// the read itself; s_mean / s_stdv / first_empty optional).  The feature rows are get_Feature's (myDetect.py:839-903), built at emit
// time.  Everything BORROWED until emit.
int dm_rows_add_mapped(dm_rowsbatch* h, int64_t n_reads, int64_t n_table_rows, int64_t n_events, int32_t n_contigs, const int64_t* bmi_off, const char* refbase, const char* readbase,
                       const int64_t* refbasei, const int64_t* start_clip, const int64_t* end_clip, const int32_t* contig,
                       const int32_t* strand, const int64_t* mev_off, const float* m_mean, const float* m_stdv, const uint64_t* m_length,
                       const char* m_base, const float* s_mean, const float* s_stdv, const int64_t* first_empty) {
    using namespace rowsbatch;
    if (!h || n_reads < 0 || !bmi_off || !refbase || !readbase || !refbasei || !start_clip || !end_clip || !contig || !strand || !mev_off ||
        !m_mean || !m_stdv || !m_length || !m_base)
        return fail(DM_EINVAL, "dm_rows_add_mapped: bad argument");
    if (h->planned) return fail(DM_ESTATE, "dm_rows_add_mapped after dm_rows_info");
    if (!offsets_ok(bmi_off, n_reads, n_table_rows) || !offsets_ok(mev_off, n_reads, n_events))
        return fail(DM_EINVAL, "dm_rows_add_mapped: an offset table decreases or runs past its array (%lld table rows, %lld events)",
                    (long long)n_table_rows, (long long)n_events);
    for (int64_t i = 0; i < n_reads; ++i)
        if (contig[i] < 0 || contig[i] >= n_contigs || (strand[i] != 0 && strand[i] != 1))
            return fail(DM_EINVAL, "dm_rows_add_mapped: read %lld has contig %d of %d, strand %d", (long long)i, contig[i], n_contigs, strand[i]);
    for (int64_t i = 0; i < n_reads; ++i) {
        auto r = std::make_unique<Read>();
        r->raw = true;
        r->contig = contig[i];
        r->strand = strand[i];
        const int64_t e0 = mev_off[i], e1 = mev_off[i + 1];
        int64_t nev = e1 - e0, nstat = 0;
        if (s_mean && s_stdv) {
            nstat = nev;
            if (first_empty && first_empty[i] < nev) {
                nstat = first_empty[i];
                if (first_empty[i] > 500) nev = first_empty[i] - 1;
            }
            if (nstat > nev) nstat = nev;
        }
        r->n_events = nev;
        r->ev_mean = m_mean + e0;
        r->ev_stdv = m_stdv + e0;
        r->ev_mean2 = s_mean ? s_mean + e0 : nullptr;
        r->ev_stdv2 = s_stdv ? s_stdv + e0 : nullptr;
        r->n_stat = nstat;
        r->ev_length = m_length + e0;
        r->ev_base = m_base + e0;
        r->start_clip = start_clip[i];
        r->end_clip = end_clip[i];
        r->refb = refbase + bmi_off[i];
        r->readb = readbase + bmi_off[i];
        r->refi = refbasei + bmi_off[i];
        r->ntab = bmi_off[i + 1] - bmi_off[i];
        h->reads.push_back(std::move(r));
    }
    return DM_OK;
}

// Sizes of the batch: feature rows R, positions / flags R + X, windows centred on a base of interest S (dm_rows_emit's compact form
// holds S + X positions / flags instead), and the per-read info (INFO = 8 int64 per read, in the order the reads
// were added: status, contig, strand, windows, rows, table rows, base mismatches, extras).  mism [n][4] (optional, cap_mism records):
// (read, table row, event, mismatches of that read) of the first mismatch of each read that has one.  Returns the number of reads.
int64_t dm_rows_info(dm_rowsbatch* h, int64_t* n_rows, int64_t* n_pos, int64_t* n_sel, int64_t* read_info, int64_t* mism, int64_t cap_mism,
                     int64_t* n_mism) {
    using namespace rowsbatch;
    if (!h) return fail(DM_EINVAL, "null batch");
    if (!h->planned) {
        h->n_rows = h->n_extra = h->n_sel = 0;
        for (auto& rp : h->reads) {
            plan_read(*rp, h->base);
            if (rp->status == OK) {
                h->n_rows += rp->nrows;
                h->n_extra += rp->extras;
                h->n_sel += rp->nsel;
            }
        }
        h->planned = true;
    }
    if (n_rows) *n_rows = h->n_rows;
    if (n_pos) *n_pos = h->n_rows + h->n_extra;
    if (n_sel) *n_sel = h->n_sel;
    int64_t nm = 0;
    for (size_t i = 0; i < h->reads.size(); ++i) {
        const Read& r = *h->reads[i];
        if (read_info) {
            int64_t* o = read_info + i * INFO;
            o[0] = r.status; o[1] = r.contig; o[2] = r.strand; o[3] = r.status == OK ? r.n_al : 0; o[4] = r.status == OK ? r.nrows : 0;
            o[5] = r.ntab; o[6] = r.mismatches; o[7] = r.status == OK ? r.extras : 0;
        }
        if (r.mismatches && mism && nm < cap_mism) {
            int64_t* o = mism + nm * 4;
            o[0] = int64_t(i); o[1] = r.first_bad_row; o[2] = r.first_bad_event; o[3] = r.mismatches;
        }
        if (r.mismatches) ++nm;
    }
    if (n_mism) *n_mism = nm;
    return int64_t(h->reads.size());
}

// Write the batch.  Reads are grouped by (contig_rank[contig], strand) - the caller ranks the contig NAMES, '+' (0) before '-' (1) -
// and keep their order inside a group.  rows [R][7]; groups [n_groups][8] = (contig, strand, row_lo, row_hi, xlo, xhi, sel_lo, sel_hi).
//   sel_row == NULL (classic form): pos / flags [R + X], one entry per feature row (0 / 0 for padding rows) then the extras
//                    (group g's at R + xlo .. R + xhi): every row's window is classified, cls[row] pairs with flags[row];
//   sel_row != NULL (compact form): sel_row [S] = the feature rows that are centres of windows on a base of interest, in row order;
//                    pos / flags [S + X]: entry i < S belongs to window sel_row[i] (its class goes to dm_summary_add_classified),
//                    the extras follow at S + xlo.  Rows whose base is not of interest appear nowhere: their flag bit 0 is clear
//                    and the summary would ignore them (myDetect.py:1091).
// contig_rank (optional) and contig_len (optional; raised to max position + 1 per contig) have n_contig_len entries; in_range (optional): 0 if a feature is outside
// +-65504 or NaN (the split-f16 kernels refuse it).  Returns the number of groups, or a negative code.
// ev3 != NULL: the DEVICE form of the feature rows (round 5; every read of the batch must be a raw read, dm_rows_device_info): instead of rows [R][7]
// the batch hands over  ev3 [E][3] = (mean, stdv, length) of the events its rows cover, in read order;  code [R] = the one-hot class of a row
// (0..3 = A, C, G, T; 255 = none: padding rows, insertions, N);  rdesc [reads][4] = (first row, row -> event shift, first event, end event) of every
// emitted read - row q of the batch belongs to the last read whose first row is <= q and shows event e = q + shift if first <= e < end, else no event.
// dm_rows_assemble turns that into the same [R][7] matrix on the device (13 instead of 28 bytes per row over PCIe, and no row is written on the host).
static int64_t rows_emit_impl(dm_rowsbatch* h, const int32_t* contig_rank, float* rows, int32_t* sel_row, int64_t* pos, uint8_t* flags,
                              int64_t* groups, int64_t cap_groups, int64_t* contig_len, int64_t n_contig_len, int32_t* in_range,
                              float* ev3, uint8_t* code, int64_t* rdesc, bool resident = false) {
    using namespace rowsbatch;
    if (!h || !h->planned) return fail(DM_ESTATE, "dm_rows_emit before dm_rows_info");
    const bool device_form = ev3 != nullptr || resident;
    {
        const int64_t n_pf = (sel_row ? h->n_sel : h->n_rows) + h->n_extra;       // entries of pos / flags in the chosen form
        if ((h->n_rows > 0 && !rows && !device_form) || (n_pf > 0 && (!pos || !flags)) || !groups) return fail(DM_EINVAL, "dm_rows_emit: null output");
        if (device_form && (!code || !rdesc)) return fail(DM_EINVAL, "dm_rows_emit_device: null output");
        if (resident != h->resident) return fail(DM_ESTATE, resident ? "dm_rows_emit_resident: the batch's reads were added with host statistics"
                                                                      : "dm_rows_emit: the statistics of the batch's reads stay on the device - dm_rows_emit_resident");
    }
    int64_t ev_out = 0, rd_out = 0;                       // events / read descriptors written so far (device form)
    std::vector<size_t> order;
    for (size_t i = 0; i < h->reads.size(); ++i)
        if (h->reads[i]->status == OK) {
            if (contig_rank && (h->reads[i]->contig < 0 || h->reads[i]->contig >= n_contig_len))
                return fail(DM_EINVAL, "dm_rows_emit: read %lld names contig %d, the rank table has %lld entries", (long long)i, h->reads[i]->contig,
                            (long long)n_contig_len);
            order.push_back(i);
        }
    auto key = [&](size_t i) {
        const Read& r = *h->reads[i];
        return std::make_pair(contig_rank ? int64_t(contig_rank[r.contig]) : int64_t(r.contig), int64_t(r.strand));
    };
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key(a) < key(b); });
    const int64_t R = h->n_rows;
    const bool compact = sel_row != nullptr;
    if (compact && R > 0x7fffffffLL) return fail(DM_EINVAL, "dm_rows_emit: %lld rows do not fit 32-bit window indices", (long long)R);
    const int64_t XB = compact ? h->n_sel : R;          // where the extras start in pos / flags
    int64_t row = 0, x = 0, ns = 0, ng = 0;
    float fmin = 0.0f, fmax = 0.0f;
    bool has_nan = false;
    for (size_t oi = 0; oi < order.size(); ++oi) {
        const Read& r = *h->reads[order[oi]];
        if (oi == 0 || key(order[oi]) != key(order[oi - 1])) {
            if (ng >= cap_groups) return fail(DM_EINVAL, "dm_rows_emit: more than %lld groups", (long long)cap_groups);
            int64_t* g = groups + ng * 8;
            g[0] = r.contig; g[1] = r.strand; g[2] = row; g[3] = row; g[4] = x; g[5] = x; g[6] = ns; g[7] = ns;
            ++ng;
        }
        int64_t* g = groups + (ng - 1) * 8;
        float* out = device_form ? nullptr : rows + row * DM_NFEAT;
        if (device_form) {
            if (!r.raw) return fail(DM_ESTATE, "dm_rows_emit_device: a read of the batch is not a raw read");
            // the events rows [0, nrows) of this read cover: ie = start_clip - PAD + q
            const int64_t ie_lo = std::max<int64_t>(0, r.start_clip - PAD), ie_hi = std::min<int64_t>(r.n_events, r.start_clip - PAD + r.nrows);
            int64_t* d = rdesc + rd_out * 4;
            ++rd_out;
            d[0] = row;
            if (resident) {
                // the statistics of event ie of this read are entry ev_first + ie of the device block the signal stage wrote (mean, stdv, length; the
                // table's fall-back values merged there): nothing per event is written here, only what the host still knows is range-checked
                d[1] = r.ev_first + (r.start_clip - PAD) - row;
                d[2] = r.ev_first + ie_lo;
                d[3] = r.ev_first + std::max(ie_lo, ie_hi);
                if (in_range) {
                    uint64_t longest = 0;                 // (a plain maximum over the length column; the few fall-back values one by one)
                    for (int64_t ie = ie_lo; ie < ie_hi; ++ie) longest = r.ev_length[ie] > longest ? r.ev_length[ie] : longest;
                    if (float(double(longest)) > fmax) fmax = float(double(longest));
                    for (int64_t ie = std::max(ie_lo, r.n_stat); ie < ie_hi; ++ie)
                        for (const float v : {r.ev_mean[ie], r.ev_stdv[ie]}) {
                            if (v != v) has_nan = true;
                            else {
                                if (v < fmin) fmin = v;
                                if (v > fmax) fmax = v;
                            }
                        }
                }
            } else {
                d[1] = (ev_out - ie_lo) + (r.start_clip - PAD) - row;      // event index of batch row q: q + d[1]
                d[2] = ev_out;
                d[3] = ev_out + std::max<int64_t>(0, ie_hi - ie_lo);
            }
            for (int64_t ie = ie_lo; !resident && ie < ie_hi; ++ie) {
                float* o = ev3 + (ev_out++) * 3;
                o[0] = ie < r.n_stat ? r.ev_mean2[ie] : r.ev_mean[ie];
                o[1] = ie < r.n_stat ? r.ev_stdv2[ie] : r.ev_stdv[ie];
                o[2] = float(double(r.ev_length[ie]));
                if (in_range)
                    for (int c = 0; c < 3; ++c) {
                        const float v = o[c];
                        if (v != v) has_nan = true;
                        else {
                            if (v < fmin) fmin = v;
                            if (v > fmax) fmax = v;
                        }
                    }
            }
            std::memset(code + row, 255, size_t(r.nrows));
        } else if (!r.raw) {
            std::memcpy(out, r.tx, sizeof(float) * size_t(r.nrows) * DM_NFEAT);
        } else {
            // get_Feature: rows cover events ie in [start_clip - 100, n_events - end_clip + 100); an existing event gives mean, stdv, length
            std::memset(out, 0, sizeof(float) * size_t(r.nrows) * DM_NFEAT);
            for (int64_t q = 0; q < r.nrows; ++q) {
                const int64_t ie = r.start_clip - PAD + q;
                if (ie < 0 || ie >= r.n_events) continue;
                float* o = out + q * DM_NFEAT;
                o[4] = ie < r.n_stat ? r.ev_mean2[ie] : r.ev_mean[ie];
                o[5] = ie < r.n_stat ? r.ev_stdv2[ie] : r.ev_stdv[ie];
                o[6] = float(double(r.ev_length[ie]));
            }
        }
        if (!compact) {
            std::memset(pos + row, 0, sizeof(int64_t) * size_t(r.nrows));
            std::memset(flags + row, 0, size_t(r.nrows));
        }
        int64_t mx = -1;
        {
            // everything the walk reads, in locals: `flags` and `code` are byte pointers - a store through one of them may alias any object, so the
            // compiler would otherwise reload the read's fields (and h->base) after every row
            const char* const t_ref = r.refb;
            const char* const t_read = r.readb;
            const int64_t* const t_pos = r.refi;
            const int64_t ntab = r.ntab, n_al = r.n_al;
            const char base = h->base;
            const bool raw_codes = r.raw;
            const int64_t d0 = row + PAD;
            uint8_t* const code_w = device_form ? code : nullptr;
            float* const rows_w = (!device_form && r.raw) ? out : nullptr;
            int64_t k = 0, xs = x, nsel = ns;
            int64_t j = 0;
            if (compact && code_w && raw_codes && r.tab_off >= 0) {     // (tab_off >= 0: the table is this library's own - dm_rows_add_mapped's are the caller's)
                // the form every batch of raw reads takes (compact window list, class bytes): the loop with its invariant choices made.  The class byte is
                // stored for every aligned row (255 = none is what the memset wrote); positions are read only for rows of the base of interest - the
                // table of a raw read was built by map_read_core, its positions never decrease ('+') or never increase ('-'), so the largest position
                // under the aligned rows is at the first or the last of them
                int64_t j_first = -1, j_last = -1;
                for (; j < ntab; ++j) {
                    const char qb = t_read[j], rb = t_ref[j];
                    if (qb != '-') {
                        if (k >= n_al) break;          // (aligned events used up: what follows can only be extras - the general loop below)
                        const int64_t d = d0 + k;
                        code_w[d] = kBaseCode.t[static_cast<unsigned char>(rb)];
                        if (rb == base) {
                            sel_row[nsel] = int32_t(d);
                            pos[nsel] = t_pos[j];
                            flags[nsel] = uint8_t(3);
                            ++nsel;
                        }
                        if (j_first < 0) j_first = j;
                        j_last = j;
                        ++k;
                    } else if (rb == base) {
                        const int64_t p = t_pos[j];
                        pos[XB + xs] = p;
                        flags[XB + xs] = uint8_t(1);
                        if (p > mx) mx = p;
                        ++xs;
                    }
                }
                if (j_first >= 0) mx = std::max(mx, std::max(t_pos[j_first], t_pos[j_last]));
            }
            for (; j < ntab; ++j) {
                const char qb = t_read[j], rb = t_ref[j];
                const bool not_gap = qb != '-';
                const bool is_base = rb == base;
                if (not_gap && k < n_al) {
                    const int64_t d = d0 + k;
                    const int64_t p = t_pos[j];
                    if (!compact) {
                        pos[d] = p;
                        flags[d] = uint8_t((is_base ? 1 : 0) | 2);
                    } else if (is_base) {
                        sel_row[nsel] = int32_t(d);
                        pos[nsel] = p;
                        flags[nsel] = uint8_t(3);
                        ++nsel;
                    }
                    if (p > mx) mx = p;
                    if (raw_codes) {       // one-hot of the (strand-corrected) reference base; '-' (insertion), N: none
                        const int c = kBaseCode.t[static_cast<unsigned char>(rb)];
                        if (c < 4) {
                            if (code_w) code_w[d] = uint8_t(c);
                            else rows_w[(PAD + k) * DM_NFEAT + c] = 1.0f;
                        }
                    }
                    ++k;
                } else {
                    if (is_base) {
                        const int64_t p = t_pos[j];
                        pos[XB + xs] = p;
                        flags[XB + xs] = uint8_t(1 | (not_gap ? 2 : 0));
                        if (p > mx) mx = p;
                        ++xs;
                    }
                    if (not_gap) ++k;
                }
            }
            x = xs;
            ns = nsel;
        }
        if (contig_len && r.contig >= 0 && r.contig < n_contig_len && mx + 1 > contig_len[r.contig]) contig_len[r.contig] = mx + 1;
        if (in_range && !device_form)
            for (int64_t q = 0; q < r.nrows * DM_NFEAT; ++q) {
                const float v = out[q];
                if (v != v) has_nan = true;
                else {
                    if (v < fmin) fmin = v;
                    if (v > fmax) fmax = v;
                }
            }
        row += r.nrows;
        g[3] = row;
        g[5] = x;
        g[7] = ns;
    }
    if (in_range) *in_range = (!has_nan && fmax <= 65504.0f && fmin >= -65504.0f) ? 1 : 0;
    return ng;
}

int64_t dm_rows_emit(dm_rowsbatch* h, const int32_t* contig_rank, float* rows, int32_t* sel_row, int64_t* pos, uint8_t* flags,
                     int64_t* groups, int64_t cap_groups, int64_t* contig_len, int64_t n_contig_len, int32_t* in_range) {
    return rows_emit_impl(h, contig_rank, rows, sel_row, pos, flags, groups, cap_groups, contig_len, n_contig_len, in_range, nullptr, nullptr, nullptr);
}

// Can the batch be handed over in the device form, and how large is it?  Returns 1 if every emitted read is a raw read (and there is at least one),
// else 0; *n_events = entries of ev3, *n_reads = rows of rdesc.  After dm_rows_info.
int dm_rows_device_info(dm_rowsbatch* h, int64_t* n_events, int64_t* n_reads) {
    using namespace rowsbatch;
    if (!h || !h->planned) return fail(DM_ESTATE, "dm_rows_device_info before dm_rows_info");
    int64_t ne = 0, nr = 0;
    bool all_raw = true;
    for (auto& rp : h->reads) {
        const Read& r = *rp;
        if (r.status != OK) continue;
        if (!r.raw) all_raw = false;
        const int64_t ie_lo = std::max<int64_t>(0, r.start_clip - PAD), ie_hi = std::min<int64_t>(r.n_events, r.start_clip - PAD + r.nrows);
        ne += std::max<int64_t>(0, ie_hi - ie_lo);
        ++nr;
    }
    if (n_events) *n_events = ne;
    if (n_reads) *n_reads = nr;
    return all_raw && nr > 0 ? 1 : 0;
}

int64_t dm_rows_emit_device(dm_rowsbatch* h, const int32_t* contig_rank, float* ev3, uint8_t* code, int64_t* rdesc, int32_t* sel_row, int64_t* pos,
                            uint8_t* flags, int64_t* groups, int64_t cap_groups, int64_t* contig_len, int64_t n_contig_len, int32_t* in_range) {
    if (!ev3) return fail(DM_EINVAL, "dm_rows_emit_device: null output");
    return rows_emit_impl(h, contig_rank, nullptr, sel_row, pos, flags, groups, cap_groups, contig_len, n_contig_len, in_range, ev3, code, rdesc);
}

// The RESIDENT form (round 6): as dm_rows_emit_device, for a batch whose reads were added with "statistics on the device" (dm_rows_add_raw with
// s_mean == s_stdv == NULL): no ev3 - rdesc's event indices point into the [n_events][3] block dm_signal_event_stats_device wrote for the batch's
// merged event tables, which dm_rows_assemble reads where it is.  The host hands over a class byte per row, a descriptor per read, the window list,
// positions and flags; in_range covers the event lengths and the table's fall-back values (the signal stage reports its own values' range).
int64_t dm_rows_emit_resident(dm_rowsbatch* h, const int32_t* contig_rank, uint8_t* code, int64_t* rdesc, int32_t* sel_row, int64_t* pos, uint8_t* flags,
                              int64_t* groups, int64_t cap_groups, int64_t* contig_len, int64_t n_contig_len, int32_t* in_range) {
    return rows_emit_impl(h, contig_rank, nullptr, sel_row, pos, flags, groups, cap_groups, contig_len, n_contig_len, in_range, nullptr, code, rdesc, true);
}

}  // extern "C"
