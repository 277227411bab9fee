// host.h - what the host-side translation units of libdeepmod_hip.so share (deepmod_hip.hip, summary.hip, feed.hip, offline.hip; DESIGN.md
// "Translation units").  Internal, not installed.  Declarations only: every object named here is defined exactly once, in deepmod_hip.hip
// (map_read_core: in readmap.inc) - a variable defined in this header would silently become one copy per unit.  The two pieces of code it
// holds are inline and own no object: DevBufs, the grow-only device blocks of a handle, and add_time.  Of dm_model it knows the name and three
// accessors (its device, its stream, whether it is asynchronous); the struct is deepmod_hip.hip's own.
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
// handles that more than one file needs: dm_summary and dm_cluster are shared by summary.hip and cluster_sites.hip.inc.  Every other handle is defined
// in the one file that uses it - dm_model in deepmod_hip.hip: the other units follow its stream (summary.hip) and read its device (offline.hip)
// through the accessors below, so a change of its fields recompiles the core unit alone.
// ---------------------------------------------------------------------------------------------
namespace dmhost {
DM_HIDDEN_SYM int model_device(const dm_model* m);
DM_HIDDEN_SYM hipStream_t model_stream(const dm_model* m);
DM_HIDDEN_SYM bool model_async(const dm_model* m);      // DM_OPT_ASYNC
}  // namespace dmhost
using dmhost::model_device;
using dmhost::model_async;
using dmhost::model_stream;

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
