// host.h - what the host-side translation units of libdeepmod_hip.so share (deepmod_hip.hip, summary.hip, feed.hip, offline.hip; DESIGN.md
// "Translation units").  Internal, not installed.  Declarations only: every object named here is defined exactly once, in deepmod_hip.hip
// (map_read_core: in readmap.inc) - a variable defined in this header would silently become one copy per unit.  The two pieces of code it
// holds are inline and own no object: DevBufs, the grow-only device blocks of a handle, and add_time.
// Without HIP (g++ on the host-only files: tests/asan/host_shim.cpp) the header is its first part alone: the C ABI and the error slot.
#pragma once

#ifdef __HIP__
#include "kernels.h"
#endif

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/deepmod_hip.h"

#define DM_HIDDEN_SYM __attribute__((visibility("hidden")))

namespace dmhost {
// the message dm_last_error() returns, per thread: ONE slot for the functions of every unit
extern DM_HIDDEN_SYM thread_local std::string g_err;
DM_HIDDEN_SYM int fail(int code, const char* fmt, ...);
}  // namespace dmhost
using dmhost::fail;
using dmhost::g_err;

namespace readmap {
// the alignment walk (readmap.inc, compiled into feed.hip): called by the row builder (rowsbatch.inc) and by getfeatures (xyrows.inc)
DM_HIDDEN_SYM int map_read_core(int flag, int64_t pos1, const char* cigar, const char* readseq, int64_t readseq_len, const char* refseq, int64_t refseq_len,
                                int64_t n_events, char* refb, char* readb, int64_t* refi, uint64_t* readi, int64_t cap, int64_t* info, int64_t* first_row,
                                int64_t* need_rows, const bool cpg_swap = true);
}  // namespace readmap

#ifdef __HIP__

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(DM_EDEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace dmhost {
DM_HIDDEN_SYM bool is_device_ptr(const void* p);
}  // namespace dmhost
using dmhost::is_device_ptr;

// The device buffers of a handle, N blocks that only grow: a block that is large enough is kept, a larger one is allocated with room to spare.
// `who` is the handle's name in the message of a failed allocation.
template <int N>
struct DevBufs {
    const char* who;
    void* buf[N] = {};
    size_t cap[N] = {};
    int ensure(int which, size_t bytes) {
        if (cap[which] >= bytes && buf[which]) return DM_OK;
        if (buf[which]) (void)hipFree(buf[which]);
        buf[which] = nullptr;
        cap[which] = 0;
        const size_t want = bytes + (bytes >> 2) + 256;                  // grow-only, a quarter ahead
        if (hipMalloc(&buf[which], want) != hipSuccess) {
            (void)hipGetLastError();
            return fail(DM_ENOMEM, "%s: hipMalloc(%zu) failed", who, want);
        }
        cap[which] = want;
        return DM_OK;
    }
    template <class T>
    T* ptr(int which) const { return static_cast<T*>(buf[which]); }
    void release() {
        for (int i = 0; i < N; ++i) {
            if (buf[i]) (void)hipFree(buf[i]);
            buf[i] = nullptr;
            cap[i] = 0;
        }
    }
};

// into += the milliseconds between two recorded events that have completed
DM_HIDDEN_SYM inline int add_time(hipEvent_t begin, hipEvent_t end, double& into) {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, begin, end));
    into += double(ms);
    return DM_OK;
}

// ---------------------------------------------------------------------------------------------
// handles that more than one file needs: dm_model crosses units (summary.hip follows its stream, offline.hip reads its device), dm_summary and
// dm_cluster are shared by summary.hip and cluster_sites.hip.inc.  Every other handle is defined in the one file that uses it.
// ---------------------------------------------------------------------------------------------
struct dm_model {
    int device = 0;
    int num_cu = 0;
    hipStream_t stream = nullptr;
    float* d_wpack = nullptr;
    float* d_bpack = nullptr;
    float* d_hpack = nullptr;
    unsigned char* d_wpack16s = nullptr;  // experiment builds (DM_WITH_F16S): split-f16 weights in the tile-major layout of the 32x32x16 kernels
    unsigned char* d_wpack16q = nullptr;  // the same weights in the 16x16x32 layout (lstm_f16q.hip.inc)
    bool f16_q = true;                    // the split-f16 modes run lstm16q::bilstm_f16q_kernel (16x16x32 MFMAs): always, except in an experiment build with DM_OPT_F16X3_SHAPE = 32
    unsigned char* d_wpack16i = nullptr;  // the same layout with int8 cross-term records (DM_PREC_F16I8)
    float i8s[24] = {};                   // its fold scales [dir][layer][gate kind]
    unsigned char* d_wpack16qi = nullptr; // DM_PREC_F16I8 in the 16x16x32 layout (lstm16q::bilstm_f16q_kernel<1>: int8 16x16x64 cross terms)
    float i8s_q[24] = {};                 // its fold scales
    float* d_wout = nullptr;              // head W[200][2] fp32 (DM_PREC_F16X3)
    float* d_scratch = nullptr;
    unsigned long long* d_dbg = nullptr;  // DM_TIMING builds only
    float* d_plogit = nullptr;            // partial logits [2 directions][plogit_tiles * 128][2], grown on demand
    int64_t plogit_tiles = 0;
    float bout[2] = {0, 0};
    int grid_cap = 0;
    int last_grid = 0;                    // DM_INFO_LAST_GRID: workgroups of the last classifier launch (launch_bilstm)
    std::vector<float> host_weights;      // canonical blob, kept for lazy packing of other precisions
    // staging for host-pointer callers
    static constexpr int64_t STAGE_WINDOWS = 65536;
    float* d_x = nullptr;
    float* d_x2 = nullptr;       // second staging buffer: H2D of batch i+1 overlaps the kernel of batch i
    hipStream_t copy_stream = nullptr;
    static constexpr int AHEAD_EVENTS = 8;      // dm_model_h2d_ahead: copy-done events, reused round robin (a wait captures the record it was queued behind)
    hipEvent_t ahead_event[AHEAD_EVENTS] = {};
    int ahead_next = 0;
    float* d_prob = nullptr;
    uint8_t* d_cls = nullptr;
    int64_t stage_rows = 0;  // capacity of d_x in floats
    // profiling
    bool profile = false;
    bool async = false;                   // DM_OPT_ASYNC: device-resident calls return after enqueue
    int precision = DM_PREC_F16X3;        // default: fastest mode that meets the 1e-4 probability tolerance
    float f16_max_abs = 0.0f;             // largest |packed weight| (x exponent scale)
    bool f16_ok = true;                   // every packed weight is a finite f16 (checked at create; else the default is DM_PREC_F32)
    bool i8_calibrated = false;           // DM_PREC_F16I8 was selected by dm_model_calibrate_i8 (for the MFMA shape of that moment)
    int len_shift = 0;                    // DM_INFO_F16_LENGTH_SHIFT
    // DM_ERANGE bookkeeping: host-mapped words the split-f16 kernels set on an input they cannot represent.  A launch writes
    // the CURRENT slot; dm_model_mark(i) ties the current slot to marker i and moves on to a free one, so that
    // dm_model_wait_mark(i) reports exactly the launches queued between the marker before it and marker i, and a later
    // batch that is still in flight cannot leak into (or be cleared by) the check of an earlier one.
    static constexpr int RANGE_SLOTS = 2 * DM_MARKS + 2;
    int* range_flag = nullptr;            // [RANGE_SLOTS]
    int* d_range_flag = nullptr;          // its device address
    int range_cur = 0;                    // slot of the launches being queued now
    int mark_slot[DM_MARKS];              // slot tied to marker i, -1: none
    std::vector<int> range_orphans;       // slots of markers that were re-recorded before anybody waited for them: checked by dm_model_sync
    bool slot_free[RANGE_SLOTS];
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    hipEvent_t marks[DM_MARKS] = {};     // dm_model_mark / dm_model_wait_mark
    size_t events_used = 0;
    double prof_ms = 0.0;
    int64_t prof_launches = 0, prof_windows = 0;
};

struct dm_summary {
    int device = 0;
    int64_t length = 0;
    int* d_counts = nullptr;  // touch | cov | mod  (+ SLACK ints: a reduce-scatter reads up to nranks - 1 positions past the last array)
    static constexpr int64_t SLACK = 64;
    int* d_oob = nullptr;
    // grow-only blocks: POS i64 [n] and FLAGS u8 [2][n] (flags | cls) stage the host arrays of an add of n positions;
    // SLICE int [3][slice_chunk] is this rank's slice of the three arrays after dm_summary_reduce_scatter
    enum { POS, FLAGS, SLICE, N_BUF };
    DevBufs<N_BUF> b{"dm_summary"};
    static constexpr int64_t STAGE_FLOOR = int64_t(1) << 20;      // positions the staging pair holds at least
    int64_t slice_chunk = 0, slice_first = 0, slice_count = -1;   // the last scatter's chunk; slice_count < 0: no scatter result held
    int* slice() const { return b.ptr<int>(SLICE); }
    hipStream_t stream = nullptr;
    dm_model* follow = nullptr;   // dm_summary_follow: enqueue on this model's stream (in-order with its launches)
};

struct dm_cluster {
    int device = 0;
    hipStream_t stream = nullptr;
    float* d_w = nullptr;
    enum { X, OUT, N_STAGE };                  // dm_cluster_predict: staging of host rows f32 [n][14] and of their results f32 [n]
    DevBufs<N_STAGE> stage{"dm_cluster_predict"};
    // dm_cluster_sites (cluster_sites.hip.inc): device buffers of the last call (csites::B_* names the slots), grown on demand, and its site counts
    static constexpr int SITE_BUFFERS = 10;
    DevBufs<SITE_BUFFERS> sites{"dm_cluster_sites"};
    int64_t n_sites = 0, n_plus = 0;
};

#endif  // __HIP__
