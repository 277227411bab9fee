// TEST INFRASTRUCTURE - not part of the product.  The host-only logic of the dm_model runtime (deepmod_amd/csrc/modelplan.inc: modelplan::RangeSlots,
// modelplan::launch_grid) under -fsanitize=address,undefined, as a program.  The program stands in for the GPU: the DM_ERANGE words live in a heap
// block of exactly RANGE_SLOTS ints (a slot index outside it is a sanitizer report), and a "launch" writes 1 into the word of the current slot if
// it is poisoned.  The three scripted sequences are those of tests/test_gpu_range_contract.py; the random walk holds the bookkeeping to a plain
// list of the poisoned launches nobody has reported yet.  tests/test_model_host.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../include/deepmod_hip.h"
#include "../deepmod_amd/csrc/modelplan.inc"

namespace {

using modelplan::RANGE_SLOTS;

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

// a model's range slots and the device that writes them
struct Device {
    std::unique_ptr<int[]> words{new int[RANGE_SLOTS]};
    modelplan::RangeSlots rs;
    Device() { rs.reset(words.get()); }
    void launch(bool poisoned) {
        const int sl = rs.current();
        CHECK(sl >= 0 && sl < RANGE_SLOTS);
        if (poisoned) words[sl] = 1;
    }
    void mark(int i) { rs.record(i); }
    bool wait(int i) { return rs.take_mark(i); }      // dm_model_wait_mark: did it raise DM_ERANGE?
    bool sync() { return rs.take_all(); }             // dm_model_sync
};

// ten batches through markers b % DM_MARKS, each marker waited for before it is recorded again; batch j alone is poisoned
void marker_of_its_batch(int j) {
    Device d;
    const int n = 10;
    std::vector<int> raised;
    for (int b = 0; b < n; ++b) {
        const int s = b % DM_MARKS;
        if (b >= DM_MARKS && d.wait(s)) raised.push_back(b - DM_MARKS);
        d.launch(b == j);
        d.mark(s);
    }
    for (int b = n > DM_MARKS ? n - DM_MARKS : 0; b < n; ++b)
        if (d.wait(b % DM_MARKS)) raised.push_back(b);
    CHECK(raised == std::vector<int>{j});
    for (int s = 0; s < DM_MARKS; ++s) CHECK(!d.wait(s));      // reported once
    CHECK(!d.sync());
}

// marker 0 recorded after the poisoned launch and again after a clean one, nobody waited in between: the violation is left to the sync
void marker_recorded_again() {
    Device d;
    d.launch(true);
    d.mark(0);
    d.launch(false);
    d.mark(0);
    CHECK(!d.wait(0));
    CHECK(d.sync());
    CHECK(!d.sync());
    CHECK(!d.wait(0));
}

// one poisoned launch, then marker 0 recorded eighteen times with no wait - more than there are range slots
void more_markers_than_slots() {
    Device d;
    d.launch(true);
    for (int k = 0; k < 18; ++k) d.mark(0);
    CHECK(d.sync());
    CHECK(!d.sync());
    CHECK(!d.wait(0));
    d.launch(false);      // markers find slots again
    d.mark(0);
    CHECK(!d.wait(0));
    d.launch(true);
    d.mark(1);
    CHECK(d.wait(1));
    CHECK(!d.sync());
}

// Random walk over launch clean | launch poisoned | mark i | wait i | sync.  The model: the poisoned launches nobody has reported yet, each with its
// number in launch order and the word it set.  An operation that reports must clear the word of at least one of them, an operation that clears
// such a word must report (a launch is reported exactly once: it leaves the list with its word), wait i may only report launches queued before
// marker i was last recorded - the later ones are still in flight -, and nothing is left after a sync.
void random_walk(uint64_t seed, int ops) {
    Device d;
    struct Poisoned {
        long seq;
        int slot;
    };
    std::vector<Poisoned> outstanding;
    long launches = 0, reports = 0, poisoned = 0;
    long mark_seq[DM_MARKS];
    for (long& s : mark_seq) s = -1;
    uint64_t state = seed;
    auto draw = [&state](int below) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return int((state >> 33) % uint64_t(below));
    };
    for (int op = 0; op < ops; ++op) {
        const int kind = draw(16), i = draw(DM_MARKS);
        if (kind < 7) {                                    // a launch, one in four poisoned
            const bool bad = draw(4) == 0;
            d.launch(bad);
            if (bad) {
                outstanding.push_back({launches, d.rs.current()});
                ++poisoned;
            }
            ++launches;
            continue;
        }
        if (kind < 11) {                                   // mark i: more often than waits, so that markers are re-recorded and slots run out
            d.mark(i);
            mark_seq[i] = launches;
            continue;
        }
        const bool is_sync = kind == 15;
        const bool reported = is_sync ? d.sync() : d.wait(i);
        bool cleared = false;
        std::vector<Poisoned> left;
        for (const Poisoned& p : outstanding) {
            if (d.words[p.slot] != 0) {
                left.push_back(p);
                continue;
            }
            cleared = true;
            if (!is_sync) CHECK(p.seq < mark_seq[i]);      // not a launch queued after the marker
        }
        CHECK(reported == cleared);
        reports += reported ? 1 : 0;
        outstanding.swap(left);
        if (is_sync) {
            CHECK(outstanding.empty());
            for (int k = 0; k < RANGE_SLOTS; ++k) CHECK(d.words[k] == 0);
        }
    }
    CHECK(d.sync() == !outstanding.empty());
    CHECK(!d.sync());
    CHECK(poisoned > ops / 16 && reports > ops / 64);      // the walk did meet violations and reports
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

void grids() {
    CHECK(modelplan::launch_grid(4198, 256) == 247);
    for (int cap : {1, 2, 128, 255, 256})
        for (int items = 1; items <= 4 * cap + 3; ++items) {
            const int grid = modelplan::launch_grid(items, cap);
            const int rounds = ceil_div(items, items < cap ? items : cap);
            if (items <= cap) CHECK(grid == items);
            CHECK(grid >= 1 && grid <= cap);
            CHECK(ceil_div(items, grid) == rounds);
            CHECK(grid == 1 || ceil_div(items, grid - 1) > rounds);      // the smallest such grid
        }
}

}  // namespace

int main() {
    marker_of_its_batch(3);
    marker_of_its_batch(9);
    marker_recorded_again();
    more_markers_than_slots();
    for (uint64_t seed : {1u, 20261021u, 77u}) random_walk(seed, 20000);
    grids();
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("MODELPLAN-ASAN-OK\n");
    return 0;
}
