// tablestage.hip.inc — what the handles of the table stages share (dm_motifs, dm_diffmod, dm_diffrep: one run per contig over dm_summary tables
// that merge filled).  HIP only: included from the handle parts of motifs.inc, diffmod.inc and diffrep.inc, never from their rule parts, which g++
// compiles as they stand.  A handle derives from TableStage and keeps its own fields; every message names the handle or the entry point (`who`).
#ifndef DM_TABLESTAGE_HIP_INC
#define DM_TABLESTAGE_HIP_INC
#include "host.h"

// the device-count check of a *_create: false after "<who>_create: no device <d>"
inline bool table_stage_device(const char* who, const int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess && device >= 0 && device < n) return true;
    (void)hipGetLastError();
    fail(DM_EDEVICE, "%s_create: no device %d", who, device);
    return false;
}

template <int N_EV, int N_BUF>
struct TableStage {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[N_EV] = {};
    DevBufs<N_BUF> b{nullptr};

    // the non-blocking stream and the events on `device`; false: the caller says what could not be made, and destroys the handle
    bool open(const int dev, const char* who) {
        device = dev;
        b.who = who;
        bool ok = hipSetDevice(dev) == hipSuccess && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
        for (hipEvent_t& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        return ok;
    }

    void shut() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        b.release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // the n tables of a run: each on the handle's device, and what their own streams still add to them is done
    int tables_ready(const char* who, dm_summary* const* tab, const int n) const {
        for (int j = 0; j < n; ++j)
            if (tab[j]->device != device) return fail(DM_EINVAL, "%s: table %d is on device %d, the handle on device %d", who, j, tab[j]->device, device);
        int rc;
        for (int j = 0; j < n; ++j)
            if ((rc = dm_summary_sync(tab[j])) != DM_OK) return rc;
        return DM_OK;
    }

    // the first `bytes` of block `which` to the host / to zero, done on return
    int fetch_block(const int which, void* dst, const size_t bytes) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemcpyAsync(dst, b.buf[which], bytes, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return DM_OK;
    }
    int zero_block(const int which, const size_t bytes) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMemsetAsync(b.buf[which], 0, bytes, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return DM_OK;
    }
};

#endif  // DM_TABLESTAGE_HIP_INC
