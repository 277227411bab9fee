// modelplan.inc — the host-only logic of the dm_model runtime (part of deepmod_hip.hip; no HIP here, so g++ compiles it as it stands and
// tests/modelplan_asan_driver.cpp drives it under the sanitizers): which DM_ERANGE word a launch writes and which marker reports it, and the
// grid of a classifier launch.
#pragma once
#include <vector>

#include "../../include/deepmod_hip.h"

namespace modelplan {

// DM_ERANGE bookkeeping (include/deepmod_hip.h, at DM_MARKS): host-mapped words the split-f16 kernels set on an input they cannot represent.  A
// launch writes the CURRENT slot; record(i) ties the current slot to marker i and moves on to a free one, so that take_mark(i) reports exactly the
// launches queued between the marker before it and marker i, and a later batch that is still in flight cannot leak into (or be cleared by) the check
// of an earlier one.  The caller orders host and device: take_mark(i) after marker i has passed, take_all() after the stream has been synchronised.
constexpr int RANGE_SLOTS = 2 * DM_MARKS + 2;

struct RangeSlots {
    int* word = nullptr;              // [RANGE_SLOTS], written by the device: read through volatile
    int cur = 0;                      // slot of the launches being queued now
    int mark_slot[DM_MARKS];          // slot tied to marker i, -1: none
    bool slot_free[RANGE_SLOTS];
    std::vector<int> orphans;         // slots of markers that were re-recorded before anybody waited for them: reported by take_all

    void reset(int* words) {
        word = words;
        cur = 0;
        for (int k = 0; k < RANGE_SLOTS; ++k) {
            word[k] = 0;
            slot_free[k] = k != 0;
        }
        for (int i = 0; i < DM_MARKS; ++i) mark_slot[i] = -1;
        orphans.clear();
    }

    // the slot the next launch writes
    int current() const { return cur; }

    // marker i was recorded: the launches queued since the marker before it wrote the current slot, which now belongs to marker i
    void record(int i) {
        if (mark_slot[i] >= 0) orphans.push_back(mark_slot[i]);      // re-recorded unwaited: take_all reports it
        int next = -1;
        for (int k = 0; k < RANGE_SLOTS && next < 0; ++k)
            if (slot_free[k]) next = k;
        if (next < 0) {
            // every slot is tied to a marker nobody waited for (more than 2 DM_MARKS + 1 recordings without a wait): marker i gets no slot and
            // the launches go on writing the current one.  take_mark(i) then reports nothing; what was queued before marker i is reported
            // later - by the next marker that finds a free slot, or by take_all - and exactly once: never silent, but not at marker i
            mark_slot[i] = -1;
            return;
        }
        mark_slot[i] = cur;
        slot_free[next] = false;
        cur = next;
    }

    // marker i has passed: did a launch it owns meet an input it cannot represent?  Its slot is cleared and free again.  A marker without a slot
    // (reported already, or left to a later marker / take_all, see record) reports nothing
    bool take_mark(int i) {
        const int sl = mark_slot[i];
        if (sl < 0) return false;
        mark_slot[i] = -1;
        slot_free[sl] = true;
        return take(sl);
    }

    // the stream has been synchronised: every slot is final - the current one, the markers', the orphans'
    bool take_all() {
        if (!word) return false;
        bool bad = take(cur);
        for (int i = 0; i < DM_MARKS; ++i) bad |= take_mark(i);
        for (int sl : orphans) {
            bad |= take(sl);
            slot_free[sl] = true;
        }
        orphans.clear();
        return bad;
    }

private:
    // the launches that wrote `slot` have finished: was it set?  The slot is cleared
    bool take(int slot) {
        volatile int* f = word + slot;
        const bool bad = *f != 0;
        *f = 0;
        return bad;
    }
};

// Workgroups of a classifier launch: work item = (tile, direction), a persistent workgroup per CU takes items round robin, `cap` workgroups at the
// most.  When the items do not fill the last round, the launch takes ceil(items / cap) rounds whatever the grid: it is sized to that many rounds
// exactly (4,198 items on 256 CUs = 17 rounds: 247 workgroups of 17 items finish when 256 workgroups of 16 or 17 would) and the CUs left over run
// whatever else is queued - the signal stage's kernels of the next batches - instead of idling through the last round (round 6)
inline int launch_grid(int items, int cap) {
    if (items <= cap) return items;
    const int rounds = (items + cap - 1) / cap;
    return (items + rounds - 1) / rounds;
}

}  // namespace modelplan
