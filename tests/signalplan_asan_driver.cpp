// TEST INFRASTRUCTURE - not part of the product.  The host-only half of the signal stage (deepmod_amd/csrc/signalplan.inc: sig::plan_events,
// sig::plan_moves, dm_signal_plan_batch) under -fsanitize=address,undefined, as a program: tests/asan/host_shim.cpp is included as it is, and every
// input table of every call lives in a heap block of exactly its size, so that a read one element outside it is a sanitizer report.  Every table of the
// plan is compared element by element with a plain per-read restatement (restate_events / restate_moves below, 128-bit arithmetic where the product
// wraps in 64), at the smallest shapes at which the arithmetic can go wrong.  tests/test_signal.py builds and runs it.
#include "asan/host_shim.cpp"

#include <memory>

namespace {

using V64 = std::vector<int64_t>;
using VU = std::vector<uint64_t>;
using VL = std::vector<long long>;
constexpr uint64_t TWO63 = uint64_t(1) << 63;
constexpr int64_t CHUNK = sig::MOVE_CHUNK;

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a block of exactly v.size() elements (new T[0] is a valid, unreadable block)
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

bool said(const char* what) { return g_err.find(what) != std::string::npos; }

// what a plan must hold, table by table
struct Want {
    int64_t n_raw = 0, n_ev = 0, n_mv = 0, n_chunks = 0;
    VL meta, evmeta, mvmeta;
    std::vector<int> ev_read;
};

bool same(const sig::BatchPlan& p, const Want& w) {
    return p.n_raw == w.n_raw && p.n_ev == w.n_ev && p.n_mv == w.n_mv && p.n_chunks == w.n_chunks && p.meta == w.meta && p.evmeta == w.evmeta &&
           p.mvmeta == w.mvmeta && p.ev_read == w.ev_read;
}

// the clamped slice [lo, hi) of one event (or of start_0 .. end_last) in a read of nr samples: the sum is taken modulo 2^64, as numpy's uint64 does
void clamp_slice(uint64_t start, uint64_t last_start, uint64_t last_length, int64_t nr, long long* lo, long long* hi) {
    const unsigned __int128 end = (unsigned __int128)last_start + last_length;
    const uint64_t wrapped = uint64_t(end & ~uint64_t(0));
    *lo = start >= uint64_t(nr) ? nr : (long long)start;
    *hi = wrapped >= uint64_t(nr) ? nr : (long long)wrapped;
}

int64_t restate_first_empty(const VU& start, const VU& length, int64_t e0, int64_t e1, int64_t nr) {
    for (int64_t e = e0; e < e1; ++e) {
        long long lo, hi;
        clamp_slice(start[e], start[e], length[e], nr, &lo, &hi);
        if (!(start[e] < uint64_t(nr)) || hi <= lo) return e - e0;
    }
    return e1 - e0;
}

Want restate_events(const V64& raw_off, const V64& ev_off, const VU& start, const VU& length, bool resident, const V64& fe_in) {
    const size_t n = raw_off.size() - 1;
    Want w;
    w.n_raw = raw_off[n];
    w.n_ev = ev_off[n];
    w.meta.assign(3 * (n + 1), 0);
    w.evmeta.assign(2 * (n + 1), 0);
    if (!resident) w.ev_read.assign(size_t(w.n_ev), -1);
    for (size_t r = 0; r < n; ++r) {
        const int64_t e0 = ev_off[r], e1 = ev_off[r + 1], nr = raw_off[r + 1] - raw_off[r];
        long long lo, hi;
        clamp_slice(start[e0], start[e1 - 1], length[e1 - 1], nr, &lo, &hi);
        w.meta[r] = raw_off[r] + lo;
        w.meta[(n + 1) + r] = raw_off[r] + hi;
        w.meta[2 * (n + 1) + r] = raw_off[r];
        w.evmeta[r] = e0;
        w.evmeta[(n + 1) + r] = resident ? std::max<int64_t>(0, std::min<int64_t>(fe_in[r], e1 - e0)) : e1 - e0;
        for (int64_t e = e0; e < e1 && !resident; ++e) w.ev_read[size_t(e)] = int(r);
    }
    w.meta[2 * (n + 1) + n] = w.n_raw;           // the sentinels: totals behind the offset tables, 0 behind lo | hi | n_stat
    w.evmeta[n] = w.n_ev;
    return w;
}

Want restate_moves(const V64& raw_off, const V64& ev_off, const V64& mv_off, const V64& first) {
    const size_t n = raw_off.size() - 1;
    Want w;
    w.n_raw = raw_off[n];
    w.n_ev = ev_off[n];
    w.n_mv = mv_off[n];
    w.meta.assign(3 * (n + 1), 0);
    w.evmeta.assign(2 * (n + 1), 0);
    w.mvmeta.assign(3 * (n + 1), 0);
    for (size_t r = 0; r < n; ++r) {
        const int64_t nr = raw_off[r + 1] - raw_off[r], len = mv_off[r + 1] - mv_off[r];
        const bool inside = first[r] >= 0 && first[r] < nr;
        w.meta[r] = raw_off[r] + (inside ? first[r] : 0);
        w.meta[(n + 1) + r] = raw_off[r + 1];
        w.meta[2 * (n + 1) + r] = raw_off[r];
        w.evmeta[r] = ev_off[r];                 // n_stat stays 0: the segmentation kernels write it
        w.mvmeta[r] = mv_off[r];
        w.mvmeta[(n + 1) + r] = w.n_chunks;
        w.mvmeta[2 * (n + 1) + r] = first[r];
        int64_t chunks = 0;                      // 4096-byte pieces counted from the 16-byte boundary at or below the table's first byte, while bytes remain
        for (int64_t at = mv_off[r] - mv_off[r] % 16; len > 0 && at < mv_off[r + 1]; at += CHUNK) ++chunks;
        w.n_chunks += chunks;
    }
    w.meta[2 * (n + 1) + n] = w.n_raw;
    w.evmeta[n] = w.n_ev;
    w.mvmeta[n] = w.n_mv;                        // the three sentinels of mv_off | chunk_off | first: total bytes, total chunks, 0
    w.mvmeta[(n + 1) + n] = w.n_chunks;
    w.mvmeta[2 * (n + 1) + n] = 0;
    return w;
}

struct Got {
    int rc;
    sig::BatchPlan p;
};

Got events(const V64& raw_off, const V64& ev_off, const VU& start, const VU& length, bool resident = false, const V64& fe_in = {}, bool have_fb = true) {
    auto ro = exact(raw_off), eo = exact(ev_off), fe = exact(fe_in);
    auto st = exact(start), ln = exact(length);
    Got g;
    g.rc = sig::plan_events(g.p, int64_t(raw_off.size()) - 1, ro.get(), eo.get(), st.get(), ln.get(), resident, resident ? fe.get() : nullptr, have_fb);
    return g;
}

Got moves(const V64& raw_off, const V64& ev_off, const V64& mv_off, const V64& first) {
    auto ro = exact(raw_off), eo = exact(ev_off), mo = exact(mv_off), fs = exact(first);
    Got g;
    g.rc = sig::plan_moves(g.p, int64_t(raw_off.size()) - 1, ro.get(), eo.get(), mo.get(), fs.get());
    return g;
}

// dm_signal_plan_batch: -> its code, first_empty into fe (a block of exactly n_reads)
int plan_batch(const V64& raw_off, const V64& ev_off, const VU& start, const VU& length, V64* fe) {
    const int64_t n = int64_t(raw_off.size()) - 1;
    auto ro = exact(raw_off), eo = exact(ev_off);
    auto st = exact(start), ln = exact(length);
    std::unique_ptr<int64_t[]> out(new int64_t[n > 0 ? n : 0]);
    const int rc = dm_signal_plan_batch(n, ro.get(), eo.get(), st.get(), ln.get(), out.get());
    if (rc == DM_OK) fe->assign(out.get(), out.get() + n);
    return rc;
}

// an accepted event-form batch in all three shapes: the host-table plan, the resident plan with the planner's own first_empty, the planner
void accepted(const V64& raw_off, const V64& ev_off, const VU& start, const VU& length, const V64& want_fe) {
    const size_t n = raw_off.size() - 1;
    Got h = events(raw_off, ev_off, start, length);
    CHECK(h.rc == DM_OK && same(h.p, restate_events(raw_off, ev_off, start, length, false, {})));
    V64 fe;
    CHECK(plan_batch(raw_off, ev_off, start, length, &fe) == DM_OK && fe == want_fe);
    for (size_t r = 0; r < n; ++r) CHECK(want_fe[r] == restate_first_empty(start, length, ev_off[r], ev_off[r + 1], raw_off[r + 1] - raw_off[r]));
    Got d = events(raw_off, ev_off, start, length, true, want_fe);
    CHECK(d.rc == DM_OK && same(d.p, restate_events(raw_off, ev_off, start, length, true, want_fe)));
    for (size_t r = 0; r < n; ++r) CHECK(d.p.n_stat()[r] == want_fe[r]);
}

}  // namespace

int main() {
    // ---- event form ----
    // 1 read, nothing empty; the tables by hand once
    accepted(V64{0, 100}, V64{0, 3}, VU{5, 20, 40}, VU{15, 20, 30}, V64{3});
    {
        Got g = events(V64{0, 100}, V64{0, 3}, VU{5, 20, 40}, VU{15, 20, 30});
        CHECK(g.rc == DM_OK && (g.p.meta == VL{5, 0, 70, 0, 0, 100}) && (g.p.evmeta == VL{0, 3, 3, 0}) && (g.p.ev_read == std::vector<int>{0, 0, 0}));
        CHECK(g.p.n_raw == 100 && g.p.n_ev == 3 && g.p.n_mv == 0 && g.p.n_chunks == 0 && g.p.mvmeta.empty());
    }
    // a read with a single event; the same event running off the read (clamped end)
    accepted(V64{0, 50}, V64{0, 1}, VU{7}, VU{9}, V64{1});
    accepted(V64{0, 50}, V64{0, 1}, VU{49}, VU{900}, V64{1});
    // 3 reads: the first empty event at index 0 (read 0: an event of length 0), in the middle (read 1: start + length wraps to an index in front of the
    // start), nowhere (read 2, whose last event runs off the read)
    {
        const V64 raw_off{0, 60, 200, 230}, ev_off{0, 3, 7, 9};
        const VU start{10, 10, 30, /**/ 0, 40, 80, 100, /**/ 2, 12};
        const VU length{0, 20, 25, /**/ 40, ~uint64_t(0) - 10, 20, 30, /**/ 10, 500};
        accepted(raw_off, ev_off, start, length, V64{0, 1, 2});
        Got g = events(raw_off, ev_off, start, length);
        CHECK((g.p.meta == VL{10, 60, 202, 0, /**/ 55, 190, 230, 0, /**/ 0, 60, 200, 230}) && (g.p.evmeta == VL{0, 3, 7, 9, /**/ 3, 4, 2, 0}));
        CHECK((g.p.ev_read == std::vector<int>{0, 0, 0, 1, 1, 1, 1, 2, 2}));
    }
    // an event start of 2^63 and more: a LARGE index - inside a read an empty event, as a read's first start an empty slice
    accepted(V64{0, 1000}, V64{0, 4}, VU{0, TWO63 + 7, 20, 30}, VU{10, 10, 10, 10}, V64{1});
    accepted(V64{0, 1000}, V64{0, 4}, VU{0, 10, 20, ~uint64_t(0) - 4}, VU{10, 10, 10, 3}, V64{3});       // the last end is 2^64 - 2: clamped to the read
    CHECK(events(V64{0, 1000}, V64{0, 4}, VU{TWO63, 10, 20, 30}, VU{10, 10, 10, 10}).rc == DM_EINVAL && said("read 0: events cover no signal (start 1000, end 40, 1000 samples)"));
    // start + length that wraps: 30 + (2^64 - 25) = 5, the end lies before the start
    CHECK(events(V64{0, 1000}, V64{0, 4}, VU{8, 10, 20, 30}, VU{2, 10, 10, ~uint64_t(0) - 24}).rc == DM_EINVAL && said("events cover no signal (start 8, end 5, 1000 samples)"));
    {   // ... and in the second of two reads, with the planner
        V64 fe;
        CHECK(plan_batch(V64{0, 10, 30}, V64{0, 1, 3}, VU{0, 12, 3}, VU{5, 4, ~uint64_t(0)}, &fe) == DM_EINVAL && said("read 1: events cover no signal (start 12, end 2, 20 samples)"));
    }
    // the resident form: first_empty below 0 and above the event count is clamped
    {
        const V64 raw_off{0, 60, 200, 230}, ev_off{0, 3, 7, 9};
        const VU start{10, 10, 30, 0, 40, 80, 100, 2, 12}, length{5, 20, 25, 40, 10, 20, 30, 10, 500};
        for (const V64& fe : {V64{-1, 9, 2}, V64{INT64_MIN, INT64_MAX, 1}, V64{3, 4, 0}}) {
            Got g = events(raw_off, ev_off, start, length, true, fe);
            CHECK(g.rc == DM_OK && same(g.p, restate_events(raw_off, ev_off, start, length, true, fe)) && g.p.ev_read.empty());
        }
        Got g = events(raw_off, ev_off, start, length, true, V64{-1, 9, 2});
        CHECK(g.p.n_stat()[0] == 0 && g.p.n_stat()[1] == 4 && g.p.n_stat()[2] == 2 && g.p.n_stat()[3] == 0);
        // an empty event without fall-back values; none empty: no fall-back values needed
        CHECK(events(raw_off, ev_off, start, length, true, V64{3, 2, 2}, false).rc == DM_EINVAL && said("read 1 has an empty event (2 of 4) and the call has no fall-back values"));
        CHECK(events(raw_off, ev_off, start, length, true, V64{-5, 4, 2}, false).rc == DM_EINVAL && said("read 0 has an empty event (0 of 3)"));
        CHECK(events(raw_off, ev_off, start, length, true, V64{3, 4, 2}, false).rc == DM_OK);
        CHECK(events(raw_off, ev_off, start, length, true, V64{3, 99, 2}, false).rc == DM_OK);
    }
    // refused batches: the present codes and messages, from the plan and from the planner alike
    {
        const VU st{1, 2, 3, 4}, ln{2, 2, 2, 2};
        V64 fe;
        CHECK(events(V64{0, 10, 20}, V64{0, 2, 2}, st, ln).rc == DM_EINVAL && said("read 1 of the batch has no events or no samples"));
        CHECK(plan_batch(V64{0, 10, 20}, V64{0, 2, 2}, st, ln, &fe) == DM_EINVAL && said("read 1 of the batch has no events or no samples"));
        CHECK(events(V64{0, 0, 20}, V64{0, 2, 4}, st, ln).rc == DM_EINVAL && said("read 0 of the batch has no events or no samples"));
        CHECK(plan_batch(V64{0, 20, 20}, V64{0, 2, 4}, st, ln, &fe) == DM_EINVAL && said("read 1 of the batch has no events or no samples"));
        CHECK(events(V64{0, 20, 10}, V64{0, 2, 4}, st, ln).rc == DM_EINVAL && said("read 1 of the batch has no events or no samples"));
        CHECK(events(V64{1, 10, 20}, V64{0, 2, 4}, st, ln).rc == DM_EINVAL && said("the offset tables of a batch start at 0"));
        CHECK(events(V64{0, 10, 20}, V64{1, 2, 4}, st, ln).rc == DM_EINVAL && said("the offset tables of a batch start at 0"));
        CHECK(plan_batch(V64{0, 10, 20}, V64{2, 2, 4}, st, ln, &fe) == DM_EINVAL && said("the offset tables of a batch start at 0"));
        CHECK(events(V64{0, 10, 0}, V64{0, 2, 4}, st, ln).rc == DM_EINVAL && said("empty batch"));
        CHECK(events(V64{0, 10, 20}, V64{0, 2, 0}, st, ln).rc == DM_EINVAL && said("empty batch"));
        sig::BatchPlan p;
        const int64_t off2[2] = {0, 1};
        CHECK(sig::plan_events(p, -1, off2, off2, st.data(), ln.data(), false, nullptr, false) == DM_EINVAL && said("negative read count"));
        CHECK(sig::plan_events(p, 0, nullptr, nullptr, nullptr, nullptr, false, nullptr, false) == DM_OK);
        CHECK(sig::plan_events(p, 1, off2, off2, nullptr, ln.data(), false, nullptr, false) == DM_EINVAL && said("null input"));
        CHECK(dm_signal_plan_batch(1, off2, nullptr, st.data(), ln.data(), nullptr) == DM_EINVAL && said("null input"));
        const uint64_t zero[1] = {0};
        CHECK(dm_signal_plan_batch(1, off2, off2, zero, ln.data(), nullptr) == DM_OK);            // first_empty is optional
        V64 many(4098);                                                                           // 4097 reads of one sample and one event each
        for (size_t i = 0; i < many.size(); ++i) many[i] = int64_t(i);
        CHECK(events(many, many, VU(4097, 0), VU(4097, 1)).rc == DM_EINVAL && said("at most 4096 reads per call (4097 given)"));
        many.pop_back();
        CHECK(events(many, many, VU(4096, 0), VU(4096, 1)).rc == DM_OK);
    }

    // ---- move form ----
    auto moved = [](const V64& raw_off, const V64& ev_off, const V64& mv_off, const V64& first) {
        Got g = moves(raw_off, ev_off, mv_off, first);
        CHECK(g.rc == DM_OK && same(g.p, restate_moves(raw_off, ev_off, mv_off, first)) && g.p.ev_read.empty());
        return g.p;
    };
    {   // tables that do not start on a 16-byte boundary: the chunks count from mv_off & ~15.  Read 1 = bytes [5, 4101): 5 + 4096 bytes from its base
        sig::BatchPlan p = moved(V64{0, 40, 90, 130}, V64{0, 3, 9, 12}, V64{0, 5, 4101, 4117}, V64{3, 0, 39});
        CHECK(p.n_chunks == 4 && p.n_mv == 4117 && (p.mvmeta == VL{0, 5, 4101, 4117, /**/ 0, 1, 3, 4, /**/ 3, 0, 39, 0}));
        CHECK((p.meta == VL{3, 40, 129, 0, /**/ 40, 90, 130, 0, /**/ 0, 40, 90, 130}) && (p.evmeta == VL{0, 3, 9, 12, 0, 0, 0, 0}));
    }
    // an empty table: no chunk (and reads without a table between reads with one share their successor's chunk offset)
    CHECK(moved(V64{0, 30}, V64{0, 1}, V64{0, 0}, V64{4}).n_chunks == 0);
    {
        sig::BatchPlan p = moved(V64{0, 30, 60, 90}, V64{0, 2, 3, 5}, V64{0, 7, 7, 20}, V64{1, 2, 3});
        CHECK(p.n_chunks == 2 && p.chunk_off()[0] == 0 && p.chunk_off()[1] == 1 && p.chunk_off()[2] == 1 && p.chunk_off()[3] == 2);
    }
    // exactly MOVE_CHUNK entries from an aligned offset: one chunk each
    CHECK(moved(V64{0, 9000}, V64{0, 5}, V64{0, CHUNK}, V64{0}).n_chunks == 1);
    CHECK(moved(V64{0, 9000, 18000}, V64{0, 5, 9}, V64{0, CHUNK, 2 * CHUNK}, V64{0, 1}).n_chunks == 2);
    CHECK(moved(V64{0, 9000, 18000}, V64{0, 5, 9}, V64{0, 16, 16 + CHUNK}, V64{0, 1}).n_chunks == 2);
    CHECK(moved(V64{0, 9000}, V64{0, 5}, V64{0, CHUNK + 1}, V64{0}).n_chunks == 2);
    // from offset 15 the aligned base lies 15 bytes in front of the table: MOVE_CHUNK - 15 entries fill one chunk exactly, one entry more (MOVE_CHUNK - 14:
    // 4097 bytes from the base) starts a second, and so does the next
    for (const int64_t len : {CHUNK - 16, CHUNK - 15, CHUNK - 14, CHUNK - 13}) {
        sig::BatchPlan p = moved(V64{0, 40, 9000}, V64{0, 3, 9}, V64{0, 15, 15 + len}, V64{3, 0});
        CHECK(p.chunk_off()[1] == 1 && p.n_chunks == 1 + (len <= CHUNK - 15 ? 1 : 2));
    }
    // `first` negative, equal to the sample count, one below it, inside: outside the read the whole signal stands in
    {
        sig::BatchPlan p = moved(V64{0, 50, 100, 150, 200, 250}, V64{0, 1, 2, 3, 4, 5}, V64{0, 3, 6, 9, 12, 15}, V64{-1, 50, 49, 20, INT64_MIN});
        CHECK(p.lo()[0] == 0 && p.lo()[1] == 50 && p.lo()[2] == 149 && p.lo()[3] == 170 && p.lo()[4] == 200);
        CHECK(p.hi()[0] == 50 && p.hi()[4] == 250 && p.first()[0] == -1 && p.first()[1] == 50 && p.first()[4] == INT64_MIN);
    }
    // the three sentinels at the ends of mv_off | chunk_off | first
    {
        sig::BatchPlan p = moved(V64{0, 9000, 18000}, V64{0, 5, 9}, V64{0, 4100, 4105}, V64{7, 9});
        CHECK(p.mv_off()[2] == 4105 && p.chunk_off()[2] == 3 && p.first()[2] == 0 && p.mvmeta.size() == 9);
    }
    // refused: decreasing move offsets, a table of 2^30 entries (the offsets alone say so), a read without samples, offsets that do not start at 0
    CHECK(moves(V64{0, 40, 90}, V64{0, 3, 9}, V64{0, 8, 7}, V64{1, 1}).rc == DM_EINVAL && said("read 1: the move offsets decrease"));
    CHECK(moves(V64{0, 40}, V64{0, 3}, V64{0, int64_t(1) << 30}, V64{1}).rc == DM_EINVAL && said("read 0: the move offsets decrease (or a table of 2^30 entries and more)"));
    CHECK(moves(V64{0, 40}, V64{0, 3}, V64{0, (int64_t(1) << 30) - 1}, V64{1}).rc == DM_OK);
    CHECK(moves(V64{0, 40, 40}, V64{0, 3, 9}, V64{0, 8, 9}, V64{1, 1}).rc == DM_EINVAL && said("read 1 of the batch has no samples (or its event offsets decrease)"));
    CHECK(moves(V64{0, 40, 90}, V64{0, 9, 3}, V64{0, 8, 9}, V64{1, 1}).rc == DM_EINVAL && said("read 1 of the batch has no samples"));
    CHECK(moves(V64{0, 40, 90}, V64{0, 3, 9}, V64{2, 8, 9}, V64{1, 1}).rc == DM_EINVAL && said("the offset tables of a batch start at 0"));
    CHECK(moves(V64{0, 40, 90}, V64{0, 3, 0}, V64{0, 8, 9}, V64{1, 1}).rc == DM_EINVAL && said("empty batch"));
    CHECK(dm_signal_move_chunk() == CHUNK);

    if (g_failed) return 1;
    std::printf("SIGNALPLAN-ASAN-OK\n");
    return 0;
}
