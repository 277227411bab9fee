// signalplan.inc — the host-only half of the signal stage (part of feed.hip, next to signal.hip.inc; no HIP here, so tests/asan/host_shim.cpp compiles
// it with g++): what a batched call works out from its offset and event tables before it touches the device.  The checks of a batch, the slice a
// read's events cover, its first empty event and the BatchPlan - the host tables signal.hip.inc uploads as they are - each exist once, here.
#pragma once
#include "host.h"

namespace sig {

constexpr int MOVE_CHUNK = 4096;          // move-table bytes per workgroup of the segmentation kernels (signal.hip.inc: MOVE_THREADS lanes x 16 bytes)
constexpr int64_t MAX_READS = 4096;       // reads per batched call

// The slice of a read its events cover, cut as numpy cuts raw[start_0 : start_last + length_last] (myDetect.py:272): uint64 arithmetic (the sum wraps),
// both ends clamped to the read.  A start or an end of 2^63 and more is a LARGE index, not a negative one.  -> false: the slice is empty
inline bool covered_slice(const uint64_t* ev_start, const uint64_t* ev_length, int64_t e0, int64_t e1, int64_t n_samples, long long* lo, long long* hi) {
    unsigned long long l = ev_start[e0], h = ev_start[e1 - 1] + ev_length[e1 - 1];
    if (l > (unsigned long long)n_samples) l = (unsigned long long)n_samples;
    if (h > (unsigned long long)n_samples) h = (unsigned long long)n_samples;
    *lo = (long long)l;
    *hi = (long long)h;
    return h > l;
}

// index, counted from e0, of the first event of [e0, e1) whose clamped slice is empty (the reference's loop stops there, myDetect.py:334-340); e1 - e0 if none
inline int64_t first_empty_event(const uint64_t* ev_start, const uint64_t* ev_length, int64_t e0, int64_t e1, int64_t n_samples) {
    for (int64_t e = e0; e < e1; ++e) {
        const unsigned long long st = ev_start[e];
        unsigned long long en = st + ev_length[e];
        if (en > (unsigned long long)n_samples) en = (unsigned long long)n_samples;
        if (st >= en) return e - e0;
    }
    return e1 - e0;
}

// the checks every batched form makes on its offset tables; `have_tables`: none of the form's other arrays is null.  A batch of 0 reads passes: the caller returns
inline int check_batch(int64_t n_reads, const int64_t* raw_off, const int64_t* ev_off, bool have_tables) {
    if (n_reads < 0) return fail(DM_EINVAL, "negative read count");
    if (n_reads == 0) return DM_OK;
    if (!raw_off || !ev_off || !have_tables) return fail(DM_EINVAL, "null input");
    if (raw_off[0] != 0 || ev_off[0] != 0) return fail(DM_EINVAL, "the offset tables of a batch start at 0");
    if (raw_off[n_reads] <= 0 || ev_off[n_reads] <= 0) return fail(DM_EINVAL, "empty batch");
    if (n_reads > MAX_READS) return fail(DM_EINVAL, "at most 4096 reads per call (%lld given)", (long long)n_reads);
    return DM_OK;
}

// ... and on read r of an event-table batch; lo / hi: its covered slice, relative to the read's first sample
inline int check_event_read(int64_t r, const int64_t* raw_off, const int64_t* ev_off, const uint64_t* ev_start, const uint64_t* ev_length, long long* lo,
                            long long* hi) {
    const int64_t e0 = ev_off[r], e1 = ev_off[r + 1], nr = raw_off[r + 1] - raw_off[r];
    if (e1 <= e0 || nr <= 0) return fail(DM_EINVAL, "read %lld of the batch has no events or no samples", (long long)r);
    if (!covered_slice(ev_start, ev_length, e0, e1, nr, lo, hi))
        return fail(DM_EINVAL, "read %lld: events cover no signal (start %lld, end %lld, %lld samples)", (long long)r, *lo, *hi, (long long)nr);
    return DM_OK;
}

// What a batched call knows before it touches the device.  The tables are [parts][n_reads + 1], laid out as the kernels read them; the last column
// of a part is its sentinel (the batch's total where the part is an offset table, 0 elsewhere).
struct BatchPlan {
    int64_t n_reads = 0, n_raw = 0, n_ev = 0, n_mv = 0, n_chunks = 0;
    std::vector<long long> meta;      // lo | hi | off: the slice of every read the order statistics see, and its first sample (absolute sample indices)
    std::vector<long long> evmeta;    // ev_off | n_stat: the events a statistics kernel computes (all of a read's outside the resident form)
    std::vector<long long> mvmeta;    // move form: mv_off | chunk_off | first
    std::vector<int> ev_read;         // host-table form: the read of every event
    long long* part(std::vector<long long>& t, int k) { return t.data() + size_t(k) * size_t(n_reads + 1); }
    long long* lo() { return part(meta, 0); }
    long long* hi() { return part(meta, 1); }
    long long* off() { return part(meta, 2); }
    long long* ev_off() { return part(evmeta, 0); }
    long long* n_stat() { return part(evmeta, 1); }
    long long* mv_off() { return part(mvmeta, 0); }
    long long* chunk_off() { return part(mvmeta, 1); }
    long long* first() { return part(mvmeta, 2); }

    // the sizes and the two tables every form has, zeroed, with their sentinels (after check_batch)
    void begin(int64_t reads, const int64_t* raw_off, const int64_t* ev_off_in) {
        n_reads = reads;
        n_raw = raw_off[reads];
        n_ev = ev_off_in[reads];
        n_mv = n_chunks = 0;
        meta.assign(size_t(3) * (reads + 1), 0);
        evmeta.assign(size_t(2) * (reads + 1), 0);
        mvmeta.clear();
        ev_read.clear();
        off()[reads] = n_raw;
        ev_off()[reads] = n_ev;
    }
};

// Event tables, host-table and resident form.  Resident: first_empty [n_reads] is an input (dm_signal_plan_batch), clamped to [0, events of the read], and
// becomes n_stat; a read with an empty event needs the call's fall-back values (have_fb).  Host-table form: n_stat = all events, ev_read is filled.
inline int plan_events(BatchPlan& p, int64_t n_reads, const int64_t* raw_off, const int64_t* ev_off, const uint64_t* ev_start, const uint64_t* ev_length,
                       bool resident, const int64_t* first_empty, bool have_fb) {
    const int rc = check_batch(n_reads, raw_off, ev_off, ev_start && ev_length);
    if (rc != DM_OK || n_reads == 0) return rc;
    p.begin(n_reads, raw_off, ev_off);
    if (!resident) p.ev_read.resize(size_t(p.n_ev));
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t e0 = ev_off[r], e1 = ev_off[r + 1];
        long long l, h;
        const int rcr = check_event_read(r, raw_off, ev_off, ev_start, ev_length, &l, &h);
        if (rcr != DM_OK) return rcr;
        p.lo()[r] = raw_off[r] + l;
        p.hi()[r] = raw_off[r] + h;
        p.off()[r] = raw_off[r];
        p.ev_off()[r] = e0;
        p.n_stat()[r] = e1 - e0;
        if (resident) {
            const int64_t fe = first_empty[r] < 0 ? 0 : std::min<int64_t>(first_empty[r], e1 - e0);
            if (fe < e1 - e0 && !have_fb)
                return fail(DM_EINVAL, "read %lld has an empty event (%lld of %lld) and the call has no fall-back values", (long long)r, (long long)fe, (long long)(e1 - e0));
            p.n_stat()[r] = fe;
        } else {
            for (int64_t e = e0; e < e1; ++e) p.ev_read[size_t(e)] = int(r);
        }
    }
    return DM_OK;
}

// Move tables: the events are cut on the device, so n_stat stays 0 here (move_scan_kernel writes it).  The normalisation slice is [first, samples) - known
// without the events; a read whose `first` lies outside its samples fails on the device (DM_MOVE_OUTSIDE) and shows no statistics: its whole signal stands
// in, so that the order statistics see an ordinary read.  Read r's table is cut into chunks of MOVE_CHUNK bytes counted from its 16-byte-aligned base.
inline int plan_moves(BatchPlan& p, int64_t n_reads, const int64_t* raw_off, const int64_t* ev_off, const int64_t* mv_off, const int64_t* first) {
    const int rc = check_batch(n_reads, raw_off, ev_off, mv_off && first);
    if (rc != DM_OK || n_reads == 0) return rc;
    if (mv_off[0] != 0) return fail(DM_EINVAL, "the offset tables of a batch start at 0");
    p.begin(n_reads, raw_off, ev_off);
    p.mvmeta.assign(size_t(3) * (n_reads + 1), 0);
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t t0 = mv_off[r], t1 = mv_off[r + 1], nr = raw_off[r + 1] - raw_off[r];
        if (t1 < t0 || t1 - t0 >= (int64_t(1) << 30)) return fail(DM_EINVAL, "read %lld: the move offsets decrease (or a table of 2^30 entries and more)", (long long)r);
        if (ev_off[r + 1] < ev_off[r] || nr <= 0) return fail(DM_EINVAL, "read %lld of the batch has no samples (or its event offsets decrease)", (long long)r);
        const int64_t f = first[r];
        p.lo()[r] = raw_off[r] + (f >= 0 && f < nr ? f : 0);
        p.hi()[r] = raw_off[r + 1];
        p.off()[r] = raw_off[r];
        p.ev_off()[r] = ev_off[r];
        p.mv_off()[r] = t0;
        p.chunk_off()[r] = p.n_chunks;
        p.first()[r] = f;
        if (t1 > t0) p.n_chunks += (t1 - (t0 & ~int64_t(15)) + MOVE_CHUNK - 1) / MOVE_CHUNK;
    }
    p.n_mv = mv_off[n_reads];
    p.mv_off()[n_reads] = p.n_mv;
    p.chunk_off()[n_reads] = p.n_chunks;
    if (p.n_chunks >= (int64_t(1) << 31)) return fail(DM_EINVAL, "move tables of %lld chunks", (long long)p.n_chunks);
    return DM_OK;
}

}  // namespace sig

extern "C" {

// Host side of a batch of reads, no device involved: the checks dm_signal_event_stats_batch makes before it uploads anything (a read with no events
// or no samples, events that cover no signal) and first_empty[r] = index of the first event of read r whose slice is empty (n events of the read if
// none).  What a feeder needs before it walks its alignments: with it the statistics themselves can stay on the device (dm_signal_event_stats_device).
int dm_signal_plan_batch(int64_t n_reads, const int64_t* raw_off, const int64_t* ev_off, const uint64_t* ev_start, const uint64_t* ev_length,
                         int64_t* first_empty) {
    const int rc = sig::check_batch(n_reads, raw_off, ev_off, ev_start && ev_length);
    if (rc != DM_OK) return rc;
    for (int64_t r = 0; r < n_reads; ++r) {
        long long l, h;
        const int rcr = sig::check_event_read(r, raw_off, ev_off, ev_start, ev_length, &l, &h);
        if (rcr != DM_OK) return rcr;
        if (first_empty) first_empty[r] = sig::first_empty_event(ev_start, ev_length, ev_off[r], ev_off[r + 1], raw_off[r + 1] - raw_off[r]);
    }
    return DM_OK;
}

int64_t dm_signal_move_chunk(void) { return sig::MOVE_CHUNK; }

}  // extern "C"
