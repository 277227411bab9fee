// deepmod_hip.hip — the core unit of libdeepmod_hip.so: the error slot every unit reports through (host.h), device and host memory helpers, the
// dm_model runtime (the struct and its block owners, create, options, the staged loop, launch_bilstm, marks, profile; its host-only logic - range
// slots, launch grid - is modelplan.inc), the int8 calibration gate, the head kernel and rows_assemble_kernel.  The other host units are
// summary.hip, feed.hip and offline.hip (interface: host.h); the three classifier kernel families are translation units of their own
// (kern_*.hip, interface: kernels.h).  __graft_entry__.build() compiles all of them in parallel (hipcc --offload-arch=gfx950 -O3 -std=c++17
// -fPIC -c) and links them.
#include "host.h"
#include "modelplan.inc"
#include "head.hip.inc"

using dmk::Packed16;
using dmk::Packed32;

// The device blocks a handle allocates once, at their exact size.  upload() leaves a block behind only when its bytes are on the device: a failed
// copy must not leave a non-null pointer to uninitialised memory (the next launch would take it for a finished block)
template <int N>
struct FixedBufs {
    const char* who;
    void* buf[N] = {};
    int alloc(int which, size_t bytes) {
        if (hipMalloc(&buf[which], bytes) == hipSuccess) return DM_OK;
        (void)hipGetLastError();
        buf[which] = nullptr;
        return fail(DM_ENOMEM, "%s: hipMalloc(%zu) failed", who, bytes);
    }
    int upload(int which, const void* src, size_t bytes) {
        int rc = alloc(which, bytes);
        if (rc) return rc;
        const hipError_t e = hipMemcpy(buf[which], src, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) return DM_OK;
        drop(which);
        return fail(DM_EDEVICE, "%s: uploading a block of %zu bytes failed: %s", who, bytes, hipGetErrorString(e));
    }
    template <class T>
    T* ptr(int which) const { return static_cast<T*>(buf[which]); }
    void drop(int which) {
        if (buf[which]) (void)hipFree(buf[which]);
        buf[which] = nullptr;
    }
    void release() {
        for (int i = 0; i < N; ++i) drop(i);
    }
};

// Device blocks of one call, in a DevBufs: released when the call returns - after the stream has drained, where work that uses them may still be queued
template <int N>
struct CallBufs {
    DevBufs<N> b;
    hipStream_t stream;
    bool in_use = false;      // set by the call once it queues work on the blocks, cleared once it has waited for the stream
    ~CallBufs() {
        if (in_use) (void)hipStreamSynchronize(stream);
        b.release();
    }
};

struct dm_model {
    int device = 0;
    int num_cu = 0;
    hipStream_t stream = nullptr;
    // what is allocated once: the fp32 packs and the scratch (DM_TIMING builds: the debug block) in model_init, the head weights W[200][2] fp32 and the
    // split-f16 weight pack of an (MFMA shape, mode) on its first launch (ensure_pack)
    enum Pack { PACK_Q, PACK_QI, PACK_S, PACK_SI, N_PACKS };      // 16x16x32 layout (lstm_f16q.hip.inc) | 32x32x16 layout of experiment builds (DM_WITH_F16S); I: int8 cross-term records (DM_PREC_F16I8)
    enum { WPACK, BPACK, HPACK, SCRATCH, DBG, WOUT, PACK0, N_FIXED = PACK0 + N_PACKS };
    FixedBufs<N_FIXED> fixed{"dm_model"};
    float i8s[N_PACKS][24] = {};          // fold scales [dir][layer][gate kind] of the int8 packs
    bool f16_q = true;                    // the split-f16 modes run lstm16q::bilstm_f16q_kernel (16x16x32 MFMAs): always, except in an experiment build with DM_OPT_F16X3_SHAPE = 32
    // what grows: staging for host-pointer callers (X2: H2D of chunk i+1 overlaps the kernel of chunk i), partial logits [2 directions][tiles * 128][2]
    enum { X, X2, PROB, CLS, PLOGIT, N_GROW };
    DevBufs<N_GROW> grow{"dm_model"};
    static constexpr int64_t STAGE_WINDOWS = 65536;
    hipStream_t copy_stream = nullptr;          // ensure_copy_stream
    static constexpr int AHEAD_EVENTS = 8;      // dm_model_h2d_ahead: copy-done events, reused round robin (a wait captures the record it was queued behind)
    hipEvent_t ahead_event[AHEAD_EVENTS] = {};
    int ahead_next = 0;
    float bout[2] = {0, 0};
    int grid_cap = 0;
    int last_grid = 0;                    // DM_INFO_LAST_GRID: workgroups of the last classifier launch (launch_bilstm)
    std::vector<float> host_weights;      // canonical blob, kept for lazy packing of other precisions
    // profiling
    bool profile = false;
    bool async = false;                   // DM_OPT_ASYNC: device-resident calls return after enqueue
    int precision = DM_PREC_F16X3;        // default: fastest mode that meets the 1e-4 probability tolerance
    float f16_max_abs = 0.0f;             // largest |packed weight| (x exponent scale)
    bool f16_ok = true;                   // every packed weight is a finite f16 (checked at create; else the default is DM_PREC_F32)
    bool i8_calibrated = false;           // DM_PREC_F16I8 was selected by dm_model_calibrate_i8 (for the MFMA shape of that moment)
    int len_shift = 0;                    // DM_INFO_F16_LENGTH_SHIFT
    // DM_ERANGE bookkeeping (modelplan.inc): the host-mapped words, their device address, and which of them the launches and the markers own
    modelplan::RangeSlots range;          // range.word: the words [modelplan::RANGE_SLOTS]
    int* d_range_flag = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    hipEvent_t marks[DM_MARKS] = {};     // dm_model_mark / dm_model_wait_mark
    size_t events_used = 0;
    double prof_ms = 0.0;
    int64_t prof_launches = 0, prof_windows = 0;
};

namespace dmhost {

int model_device(const dm_model* m) { return m->device; }
hipStream_t model_stream(const dm_model* m) { return m->stream; }
bool model_async(const dm_model* m) { return m->async; }

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // clear sticky "invalid value" for plain host memory
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

}  // namespace dmhost

namespace {

// ---------------------------------------------------------------------------------------------
// feature rows of raw reads, assembled on the device (round 5; get_Feature, myDetect.py:839-903, fnum = 7): row q of the batch = one-hot of
// its reference base | mean, stdv, length of the event it shows - from the device form of rowsbatch.inc (ev3, code, rdesc).  HBM-bound:
// 13 B in, 28 B out per row; one thread per row, the read of a row found by binary search over the (few hundred) read descriptors.
// ---------------------------------------------------------------------------------------------
__global__ void rows_assemble_kernel(float* __restrict__ rows, const unsigned char* __restrict__ code, const float* __restrict__ ev3,
                                     const long long* __restrict__ rdesc, const int n_reads, const long long n_rows) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_rows) return;
    int lo = 0, hi = n_reads - 1;                    // the last read whose first row is <= q
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rdesc[4 * (long long)mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    const long long* d = rdesc + 4 * (long long)lo;
    const long long e = q + d[1];
    const bool has = e >= d[2] && e < d[3];
    const unsigned c = code[q];
    float* o = rows + q * DM_NFEAT;
    o[0] = c == 0u ? 1.0f : 0.0f;
    o[1] = c == 1u ? 1.0f : 0.0f;
    o[2] = c == 2u ? 1.0f : 0.0f;
    o[3] = c == 3u ? 1.0f : 0.0f;
    o[4] = has ? ev3[3 * e] : 0.0f;
    o[5] = has ? ev3[3 * e + 1] : 0.0f;
    o[6] = has ? ev3[3 * e + 2] : 0.0f;
}

int flush_profile(dm_model* m) {
    for (size_t i = 0; i < m->events_used; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(m->events[i].second));
        HIP_TRY(hipEventElapsedTime(&ms, m->events[i].first, m->events[i].second));
        m->prof_ms += ms;
    }
    m->events_used = 0;
    return DM_OK;
}

// partial-logit block of direction-split launches: 16 B per window, grown on demand (a running launch may still use the old block: wait for
// the stream before it is freed).  The block's own capacity is the record of its size: ntiles + ntiles / 4 tiles after a growth, 1,280 at least
int ensure_plogit(dm_model* m, int64_t ntiles) {
    const size_t bytes = size_t(std::max<int64_t>(ntiles, 1024)) * lstmhead::TILE_M * 2 * 2 * sizeof(float);
    if (m->grow.cap[dm_model::PLOGIT] >= bytes) return DM_OK;
    HIP_TRY(hipStreamSynchronize(m->stream));
    return m->grow.ensure(dm_model::PLOGIT, bytes);
}

// the copy stream, on first need: the staged uploads of predict_common and dm_model_h2d_ahead
int ensure_copy_stream(dm_model* m) {
    if (!m->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&m->copy_stream, hipStreamNonBlocking));
    return DM_OK;
}

// What a split-f16 launch needs, built on first use: weights that fit an f16 after the exponent-scale fold (checked once in model_init), the fp32
// head weights, the kernel prepared and the weight pack of its (shape, mode)
int ensure_pack(dm_model* m, int pack) {
    if (m->fixed.buf[dm_model::PACK0 + pack]) return DM_OK;
    if (!m->f16_ok)
        return fail(DM_EINVAL, "DM_PREC_F16X3: a packed weight (|w| x exponent scale = %g) is outside the f16 range; use DM_PREC_F32",
                    double(m->f16_max_abs));
    if (!m->fixed.buf[dm_model::WOUT]) {
        int rc = m->fixed.upload(dm_model::WOUT, m->host_weights.data() + (DM_WEIGHT_FLOATS - 402), 400 * sizeof(float));
        if (rc) return rc;
    }
    const bool i8 = pack == dm_model::PACK_QI || pack == dm_model::PACK_SI;
    hipError_t prepared;
    Packed16 P;
    if (pack == dm_model::PACK_Q || pack == dm_model::PACK_QI) {
        prepared = dmk::f16q_prepare(i8 ? 1 : 0);
        P = dmk::pack_weights_f16q(m->host_weights.data(), i8, i8 ? m->i8s[pack] : nullptr);
    } else {
#ifdef DM_WITH_F16S
        prepared = dmk::f16s_prepare(i8 ? 1 : 0);
        if (!i8 && dmk::f16s_has_roles() && dmk::f16s_prepare(2) != hipSuccess) return fail(DM_EDEVICE, "the roles kernel cannot be prepared");
        P = dmk::pack_weights_f16s(m->host_weights.data(), i8, i8 ? m->i8s[pack] : nullptr);
#else
        return fail(DM_EINVAL, "the 32x32x16 kernels are not part of this build (tools/experiments/f16s: DM_WITH_F16S=1)");
#endif
    }
    if (prepared != hipSuccess) return fail(DM_EDEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(prepared));
    return m->fixed.upload(dm_model::PACK0 + pack, P.w.data(), P.w.size());
}

// launch on device-resident buffers
int launch_bilstm(dm_model* m, const float* d_x, long long xstride, int64_t n, float* d_prob, uint8_t* d_cls, const int* d_widx = nullptr) {
    if (n <= 0) return DM_OK;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (m->profile) {
        if (m->events_used == m->events.size()) {
            if (m->events.size() >= 4096) {
                int rc = flush_profile(m);
                if (rc) return rc;
            } else {
                hipEvent_t a, b;
                HIP_TRY(hipEventCreate(&a));
                HIP_TRY(hipEventCreate(&b));
                m->events.emplace_back(a, b);
            }
        }
        e0 = m->events[m->events_used].first;
        e1 = m->events[m->events_used].second;
        ++m->events_used;
        HIP_TRY(hipEventRecord(e0, m->stream));
    }
    const int ntiles = int((n + dmk::TILE_M - 1) / dmk::TILE_M);
    {
        int rcp = ensure_plogit(m, ntiles);
        if (rcp) return rcp;
    }
    const long long npad = (long long)ntiles * dmk::TILE_M;
    const int grid = modelplan::launch_grid(2 * ntiles, m->grid_cap);      // work item = (tile, direction)
    m->last_grid = grid;
    float* const plogit = m->grow.ptr<float>(dm_model::PLOGIT);
    if (m->precision == DM_PREC_F16X3 || m->precision == DM_PREC_F16I8 || m->precision == DM_PREC_F16X3_ROLES) {
        const bool i8 = m->precision == DM_PREC_F16I8;
        const bool q = m->f16_q && m->precision != DM_PREC_F16X3_ROLES;      // DM_OPT_F16X3_SHAPE picks the MFMA shape of both modes
        const int pack = (q ? dm_model::PACK_Q : dm_model::PACK_S) + (i8 ? 1 : 0);
        int rc = ensure_pack(m, pack);
        if (rc) return rc;
        dmk::F16Args a;
        a.wpack = m->fixed.ptr<unsigned char>(dm_model::PACK0 + pack);
        a.hpack = m->fixed.ptr<float>(dm_model::WOUT);
        a.x = d_x;
        a.xstride = xstride;
        a.widx = d_widx;
        a.n = n;
        a.ntiles = ntiles;
        a.plogit = plogit;
        a.len_shift = m->len_shift;
        a.range_flag = m->d_range_flag + m->range.current();
        a.i8s = i8 ? m->i8s[pack] : nullptr;
        if (q) dmk::f16q_launch(i8 ? 1 : 0, a, grid, m->stream);
#ifdef DM_WITH_F16S
        else dmk::f16s_launch(i8 ? 1 : (m->precision == DM_PREC_F16X3_ROLES ? 2 : 0), a, grid, m->stream);
#endif
    } else {
        dmk::F32Args a;
        a.wpack = m->fixed.ptr<float>(dm_model::WPACK);
        a.bpack = m->fixed.ptr<float>(dm_model::BPACK);
        a.hpack = m->fixed.ptr<float>(dm_model::HPACK);
        a.bout0 = m->bout[0];
        a.bout1 = m->bout[1];
        a.x = d_x;
        a.xstride = xstride;
        a.widx = d_widx;
        a.n = n;
        a.prob = d_prob;
        a.cls = d_cls;
        a.scratch = m->fixed.ptr<float>(dm_model::SCRATCH);
        a.ntiles = ntiles;
        a.dbg = m->fixed.ptr<unsigned long long>(dm_model::DBG);
        a.dir_split = 1;      // work item = (tile, direction), see above
        a.plogit = plogit;
        dmk::f32_launch(a, grid, m->stream);
    }
#ifndef DM_ABL_NOHEAD      // timing only (prob / cls stay unwritten): what the finishing kernel and the dependency bubble in front of it cost a step - the most a kernel that finishes its own windows could gain
    hipLaunchKernelGGL(lstmhead::head_finish_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, m->stream, plogit, (long long)n,
                       npad, m->bout[0], m->bout[1], d_prob, d_cls);
#endif
    HIP_TRY(hipGetLastError());
    if (m->profile) {
        HIP_TRY(hipEventRecord(e1, m->stream));
        ++m->prof_launches;
        m->prof_windows += n;
    }
    return DM_OK;
}

int range_error(dm_model* m) {
    return fail(DM_ERANGE, "DM_PREC_F16X3: an input feature is outside the representable range (features 0-5: |x| <= 65504, "
                "feature 6: |x| <= 65504 * 2^%d, no NaN); the results of these launches are invalid - repeat them with DM_PREC_F32",
                m->len_shift);
}
// wait for the model's stream: every range slot is final then
int sync_and_check(dm_model* m) {
    HIP_TRY(hipStreamSynchronize(m->stream));
    return m->range.take_all() ? range_error(m) : DM_OK;
}

// windows [off, off + STAGE_WINDOWS) of the n host windows x -> dst on the copy stream (beside the launches of the model's stream); the host waits for it
int upload_chunk(dm_model* m, float* dst, const float* x, int64_t off, int64_t n) {
    const int64_t cnt = std::min<int64_t>(dm_model::STAGE_WINDOWS, n - off), win_floats = DM_WINDOW * DM_NFEAT;
    HIP_TRY(hipMemcpyAsync(dst, x + off * win_floats, sizeof(float) * cnt * win_floats, hipMemcpyHostToDevice, m->copy_stream));
    HIP_TRY(hipStreamSynchronize(m->copy_stream));
    return DM_OK;
}

int predict_common(dm_model* m, const float* x, long long xstride, int64_t x_floats_total, int64_t n,
                   float* prob, uint8_t* cls, bool windows_materialised) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (n < 0) return fail(DM_EINVAL, "negative window count");
    if (n == 0) return DM_OK;
    if (!x) return fail(DM_EINVAL, "null input");
    HIP_TRY(hipSetDevice(m->device));
    const bool xdev = is_device_ptr(x);
    const bool pdev = prob ? is_device_ptr(prob) : true;
    const bool cdev = cls ? is_device_ptr(cls) : true;
    if (xdev && pdev && cdev) {
        int rc = launch_bilstm(m, x, xstride, n, prob, cls);
        if (rc) return rc;
        if (!m->async) return sync_and_check(m);
        return DM_OK;
    }
    // a host array among them: chunks of STAGE_WINDOWS, each classified, its results copied back and waited for.  How x gets to the device is the
    // one thing the two forms differ in: it is there already (NONE); per-read rows are copied whole ahead of the loop, on the model's stream
    // (WHOLE); materialised windows go chunk by chunk through two blocks on the copy stream, chunk i + 1 while chunk i is classified (CHUNKS)
    enum Feed { NONE, WHOLE, CHUNKS };
    const Feed feed = xdev ? NONE : windows_materialised ? CHUNKS : WHOLE;
    const int64_t chunk_floats = int64_t(dm_model::STAGE_WINDOWS) * DM_WINDOW * DM_NFEAT;
    int rc = DM_OK;
    if (feed != NONE) rc = m->grow.ensure(dm_model::X, sizeof(float) * (feed == WHOLE ? x_floats_total : chunk_floats));
    if (rc == DM_OK && feed == CHUNKS) rc = m->grow.ensure(dm_model::X2, sizeof(float) * chunk_floats);
    if (rc == DM_OK && feed == CHUNKS) rc = ensure_copy_stream(m);
    if (rc == DM_OK && prob && !pdev) rc = m->grow.ensure(dm_model::PROB, sizeof(float) * 2 * dm_model::STAGE_WINDOWS);
    if (rc == DM_OK && cls && !cdev) rc = m->grow.ensure(dm_model::CLS, dm_model::STAGE_WINDOWS);
    if (rc) return rc;
    float* const stage[2] = {m->grow.ptr<float>(dm_model::X), m->grow.ptr<float>(dm_model::X2)};
    float* const d_prob = m->grow.ptr<float>(dm_model::PROB);
    uint8_t* const d_cls = m->grow.ptr<uint8_t>(dm_model::CLS);
    if (feed == WHOLE) HIP_TRY(hipMemcpyAsync(stage[0], x, sizeof(float) * x_floats_total, hipMemcpyHostToDevice, m->stream));
    if (feed == CHUNKS && (rc = upload_chunk(m, stage[0], x, 0, n))) return rc;      // prime the pipeline
    int b = 0;
    for (int64_t off = 0; off < n; off += dm_model::STAGE_WINDOWS, b ^= 1) {
        const int64_t cnt = std::min<int64_t>(dm_model::STAGE_WINDOWS, n - off);
        const float* dx = feed == CHUNKS ? stage[b] : (feed == WHOLE ? stage[0] : x) + off * xstride;
        float* dp = prob ? (pdev ? prob + 2 * off : d_prob) : nullptr;
        uint8_t* dc = cls ? (cdev ? cls + off : d_cls) : nullptr;
        rc = launch_bilstm(m, dx, xstride, cnt, dp, dc);          // asynchronous on the model's stream
        if (rc) return rc;
        const int64_t noff = off + dm_model::STAGE_WINDOWS;
        if (feed == CHUNKS && noff < n && (rc = upload_chunk(m, stage[b ^ 1], x, noff, n))) return rc;      // the next chunk meanwhile
        if (prob && !pdev) HIP_TRY(hipMemcpyAsync(prob + 2 * off, d_prob, sizeof(float) * 2 * cnt, hipMemcpyDeviceToHost, m->stream));
        if (cls && !cdev) HIP_TRY(hipMemcpyAsync(cls + off, d_cls, cnt, hipMemcpyDeviceToHost, m->stream));
        rc = sync_and_check(m);
        if (rc) return rc;
    }
    return DM_OK;
}

int model_init(dm_model* m, const float* weights) {
    HIP_TRY(hipSetDevice(m->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, m->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DM_EDEVICE, "device %d is %s; this library is built for gfx950 only", m->device, prop.gcnArchName);
    m->num_cu = prop.multiProcessorCount;
    m->grid_cap = m->num_cu;  // 120 KB of LDS per workgroup -> one resident (persistent) workgroup per CU
    HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    m->host_weights.assign(weights, weights + DM_WEIGHT_FLOATS);
    Packed32 P = dmk::pack_weights_f32(weights);
    m->bout[0] = P.bout[0];
    m->bout[1] = P.bout[1];
    int rc = m->fixed.upload(dm_model::WPACK, P.w.data(), P.w.size() * sizeof(float));
    if (rc == DM_OK) rc = m->fixed.upload(dm_model::BPACK, P.b.data(), P.b.size() * sizeof(float));
    if (rc == DM_OK) rc = m->fixed.upload(dm_model::HPACK, P.h.data(), P.h.size() * sizeof(float));
    const size_t scratch_bytes = size_t(m->grid_cap) * dmk::f32_scratch_floats_per_wg() * sizeof(float);      // h sequences of the fp32 kernel
    if (rc == DM_OK) rc = m->fixed.alloc(dm_model::SCRATCH, scratch_bytes);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(m->fixed.buf[dm_model::SCRATCH], 0, scratch_bytes, m->stream));      // ordered with the launches of m->stream (non-blocking)
#if defined(DM_TIMING) || defined(DM_TRACE) || defined(DM_TRACE2)
    const size_t dbg_bytes = size_t(m->grid_cap) * dmk::f32_waves() * 8 * sizeof(unsigned long long);
    if ((rc = m->fixed.alloc(dm_model::DBG, dbg_bytes))) return rc;
    HIP_TRY(hipMemsetAsync(m->fixed.buf[dm_model::DBG], 0, dbg_bytes, m->stream));
#endif
    HIP_TRY(dmk::f32_prepare());
    int* words = nullptr;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&words), sizeof(int) * modelplan::RANGE_SLOTS, hipHostMallocMapped));
    m->range.reset(words);
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&m->d_range_flag), words, 0));
    {   // trained kernels far outside the usual range cannot be split into f16 halves: such a model runs the fp32 kernel
        Packed16 P16 = dmk::pack_weights_f16q(weights);
        m->f16_ok = P16.finite && P16.max_abs <= 65504.0f;
        m->f16_max_abs = P16.finite ? P16.max_abs : INFINITY;
        m->len_shift = P16.len_shift;
        m->precision = m->f16_ok ? DM_PREC_F16X3 : DM_PREC_F32;
    }
    m->f16_q = true;
#ifdef DM_WITH_F16S
    {   // experiment builds: DM_F16X3_SHAPE=32 in the environment at model creation runs the split-f16 modes on the 32x32x16 kernels of rounds 2-3
        const char* e = std::getenv("DM_F16X3_SHAPE");
        m->f16_q = DM_F16X3_SHAPE_DEFAULT == 16;
        if (e && *e) {
            if (!std::strcmp(e, "16")) m->f16_q = true;
            else if (!std::strcmp(e, "32")) m->f16_q = false;
            else std::fprintf(stderr, "deepmod_hip: DM_F16X3_SHAPE=%s ignored (16 or 32); the default shape %d stays\n", e, DM_F16X3_SHAPE_DEFAULT);
        }
    }
#endif
    return DM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

const char* dm_last_error(void) { return g_err.c_str(); }
#define DM_STR2(X) #X
#define DM_STR(X) DM_STR2(X)
// the compiler is part of the identity of the hand-scheduled kernels: the evidence of a round is valid for the hipcc it was taken with
const char* dm_version(void) { return "deepmod_hip 0.5 (gfx950; hip " DM_STR(HIP_VERSION_MAJOR) "." DM_STR(HIP_VERSION_MINOR) "." DM_STR(HIP_VERSION_PATCH) "; " __VERSION__ ")"; }
const char* dm_build_flags(void) {
#ifdef DM_EXPERIMENT
    return "experiment=1 switches=" DM_STR(DM_ANY_EXPERIMENT_SWITCH);
#else
    return "experiment=0 switches=0";
#endif
}

int dm_device_pci_bus_id(int device, char* buf, int len) {
    if (!buf || len < 13) return fail(DM_EINVAL, "dm_device_pci_bus_id: buffer of >= 13 bytes");
    HIP_TRY(hipDeviceGetPCIBusId(buf, len, device));
    return DM_OK;
}

int dm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int ok = 0;
    for (int d = 0; d < n; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

dm_model* dm_model_create(int device, const float* weights, size_t n_floats, int n_feat, int hidden, int window,
                          int layers) {
    if (!weights || n_floats != DM_WEIGHT_FLOATS) {
        fail(DM_EINVAL, "weights: expected %d floats, got %zu", DM_WEIGHT_FLOATS, n_floats);
        return nullptr;
    }
    if (n_feat != DM_NFEAT || hidden != DM_HIDDEN || window != DM_WINDOW || layers != DM_LAYERS) {
        fail(DM_EINVAL, "unsupported geometry fnum=%d hidden=%d window=%d layers=%d (built for 7/100/21/3)", n_feat,
             hidden, window, layers);
        return nullptr;
    }
    dm_model* m = new (std::nothrow) dm_model();
    if (!m) {
        fail(DM_ENOMEM, "out of host memory");
        return nullptr;
    }
    m->device = device;
    if (model_init(m, weights) != DM_OK) {
        std::string keep = g_err;
        dm_model_destroy(m);
        g_err = keep;
        return nullptr;
    }
    return m;
}

void dm_model_destroy(dm_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (auto& e : m->events) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    for (hipEvent_t e : m->marks)
        if (e) (void)hipEventDestroy(e);
    m->fixed.release();
    m->grow.release();
    for (hipEvent_t ev : m->ahead_event)
        if (ev) (void)hipEventDestroy(ev);
    if (m->copy_stream) (void)hipStreamDestroy(m->copy_stream);
    if (m->range.word) (void)hipHostFree(m->range.word);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

int dm_model_set_option(dm_model* m, int key, int64_t value) {
    if (!m) return fail(DM_EINVAL, "null model");
    switch (key) {
        case DM_OPT_PROFILE:
            m->profile = value != 0;
            return DM_OK;
        case DM_OPT_ASYNC:
            m->async = value != 0;
            return DM_OK;
        case DM_OPT_F16X3_SHAPE:
            if (value != 16 && value != 32) return fail(DM_EINVAL, "DM_OPT_F16X3_SHAPE: %lld (16 or 32)", (long long)value);
#ifndef DM_WITH_F16S
            if (value == 32)
                return fail(DM_EINVAL, "DM_OPT_F16X3_SHAPE = 32 (the 32x32x16 kernels of rounds 2-3) is not part of this build: tools/experiments/f16s, DM_WITH_F16S=1");
#endif
            if ((value == 16) != m->f16_q && m->precision == DM_PREC_F16I8 && m->i8_calibrated) {
                // the calibration gate looked at the int8 kernel of the OTHER shape (its own pack, its own quantisation): the selection does not carry over
                m->precision = DM_PREC_F16X3;
                m->i8_calibrated = false;
            }
            m->f16_q = value == 16;
            return DM_OK;
        case DM_OPT_RESERVED_CUS:
            if (value < 0 || value > m->num_cu / 2) return fail(DM_EINVAL, "reserved CUs %lld outside [0, %d]", (long long)value, m->num_cu / 2);
            m->grid_cap = m->num_cu - int(value);
            return DM_OK;
        case DM_OPT_PRECISION:
            if (value != DM_PREC_F32 && value != DM_PREC_F16X3 && value != DM_PREC_F16X3_ROLES && value != DM_PREC_F16I8)
                return fail(DM_EINVAL, "unknown precision %lld", (long long)value);
            m->i8_calibrated = false;      // an explicit choice of the caller
#ifndef DM_WITH_F16X3_ROLES
            if (value == DM_PREC_F16X3_ROLES)
                return fail(DM_EINVAL, "DM_PREC_F16X3_ROLES (the wave-pair experiment kernel of round 4) is not part of this build; rebuild with -DDM_WITH_F16X3_ROLES");
#endif
            if (value != DM_PREC_F32 && !m->f16_ok)
                return fail(DM_EINVAL, "DM_PREC_F16X3 refused: a packed weight of this model is outside the f16 range (|w| x 2.886 > 65504)");
            m->precision = int(value);
            return DM_OK;
        default:
            return fail(DM_EINVAL, "unknown option %d", key);
    }
}

int dm_predict_windows(dm_model* m, const float* x, int64_t n, float* prob, uint8_t* cls) {
    return predict_common(m, x, DM_WINDOW * DM_NFEAT, n * DM_WINDOW * DM_NFEAT, n, prob, cls, true);
}

int dm_predict_read(dm_model* m, const float* rows, int64_t m_rows, int64_t first, int64_t count, float* prob,
                    uint8_t* cls) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (count < 0 || first < DM_WINDOW / 2 || first + count + DM_WINDOW / 2 > m_rows)
        return fail(DM_EINVAL, "window range [%lld, %lld) +-10 outside the %lld feature rows", (long long)first,
                    (long long)(first + count), (long long)m_rows);
    if (count == 0) return DM_OK;
    if (!rows) return fail(DM_EINVAL, "null input");
    // window i = rows[first + i - 10 .. first + i + 10]  ->  base pointer at row (first - 10), window stride 7
    if (is_device_ptr(rows))
        return predict_common(m, rows + (first - DM_WINDOW / 2) * DM_NFEAT, DM_NFEAT, 0, count, prob, cls, false);
    // host rows: ship only the rows this call needs
    const float* base = rows + (first - DM_WINDOW / 2) * DM_NFEAT;
    return predict_common(m, base, DM_NFEAT, (count + DM_WINDOW - 1) * DM_NFEAT, count, prob, cls, false);
}

// Classify `count` windows of a feature-row matrix picked by their CENTRE rows: window i = rows[centre[i] - 10 .. centre[i] + 10].
// What the streaming worker calls: only windows centred on a base of interest can reach the BED (sum_handler tests refbase == Base
// before it looks at mod_pred, myDetect.py:1091-1100), so the other ~3/4 of a read's windows are never computed.  Everything
// device-resident: queued on the model's stream (DM_OPT_ASYNC), else synchronous.  Host arrays are staged through temporaries.
int dm_predict_read_at(dm_model* m, const float* rows, int64_t m_rows, const int32_t* centre, int64_t count, float* prob, uint8_t* cls) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (count < 0 || m_rows < 0) return fail(DM_EINVAL, "negative count");
    if (count == 0) return DM_OK;
    if (!rows || !centre) return fail(DM_EINVAL, "null input");
    if (m_rows < DM_WINDOW) return fail(DM_EINVAL, "%lld feature rows hold no window", (long long)m_rows);
    HIP_TRY(hipSetDevice(m->device));
    const bool rd = is_device_ptr(rows), cd = is_device_ptr(centre), pd = prob ? is_device_ptr(prob) : true, kd = cls ? is_device_ptr(cls) : true;
    if (rd && cd && pd && kd) {
        int rc = launch_bilstm(m, rows - (DM_WINDOW / 2) * DM_NFEAT, DM_NFEAT, count, prob, cls, centre);
        if (rc) return rc;
        return m->async ? DM_OK : sync_and_check(m);
    }
    // host arrays (tests, small callers): the centres are checked, everything goes through temporaries, synchronous
    if (!cd)
        for (int64_t i = 0; i < count; ++i)
            if (centre[i] < DM_WINDOW / 2 || centre[i] >= m_rows - DM_WINDOW / 2)
                return fail(DM_EINVAL, "window %lld: centre row %d +-10 outside the %lld feature rows", (long long)i, centre[i], (long long)m_rows);
    enum { ROWS, CENTRE, PROB, CLS, N_TMP };
    CallBufs<N_TMP> tmp{{"dm_predict_read_at"}, m->stream};
    int rc = DM_OK;
    if (!rd) rc = tmp.b.ensure(ROWS, sizeof(float) * size_t(m_rows) * DM_NFEAT);
    if (rc == DM_OK && !cd) rc = tmp.b.ensure(CENTRE, sizeof(int) * size_t(count));
    if (rc == DM_OK && prob && !pd) rc = tmp.b.ensure(PROB, sizeof(float) * 2 * size_t(count));
    if (rc == DM_OK && cls && !kd) rc = tmp.b.ensure(CLS, size_t(count));
    if (rc) return rc;
    const float* d_rows = rd ? rows : tmp.b.ptr<float>(ROWS);
    const int* d_centre = cd ? centre : tmp.b.ptr<int>(CENTRE);
    float* d_prob = prob && !pd ? tmp.b.ptr<float>(PROB) : prob;
    uint8_t* d_cls = cls && !kd ? tmp.b.ptr<uint8_t>(CLS) : cls;
    tmp.in_use = true;      // from here on a return waits for the stream before the temporaries go, a failed launch included
    if (!rd) HIP_TRY(hipMemcpyAsync(tmp.b.buf[ROWS], rows, sizeof(float) * size_t(m_rows) * DM_NFEAT, hipMemcpyHostToDevice, m->stream));
    if (!cd) HIP_TRY(hipMemcpyAsync(tmp.b.buf[CENTRE], centre, sizeof(int) * size_t(count), hipMemcpyHostToDevice, m->stream));
    rc = launch_bilstm(m, d_rows - (DM_WINDOW / 2) * DM_NFEAT, DM_NFEAT, count, d_prob, d_cls, d_centre);
    if (rc) return rc;
    if (prob && !pd) HIP_TRY(hipMemcpyAsync(prob, d_prob, sizeof(float) * 2 * size_t(count), hipMemcpyDeviceToHost, m->stream));
    if (cls && !kd) HIP_TRY(hipMemcpyAsync(cls, d_cls, size_t(count), hipMemcpyDeviceToHost, m->stream));
    rc = sync_and_check(m);
    tmp.in_use = false;
    return rc;
}

// debug builds (-DDM_TIMING): copy the per-wave section cycle counters [grid][waves][8]; returns element count
extern "C" long long dm_debug_timing(dm_model* m, unsigned long long* out, long long cap) {
    if (!m || !m->fixed.buf[dm_model::DBG]) return 0;
    const long long n = (long long)m->grid_cap * dmk::f32_waves() * 8;
    if (out && cap >= n) (void)hipMemcpy(out, m->fixed.buf[dm_model::DBG], n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    return n;
}

// ---- load-time calibration gate of the opt-in int8 mode (round 4) ----
// windows with the distribution of BASELINE configs[1] (deepmod_amd/synth.py synthetic_windows: base one-hot 4 x 24 % + 4 % none, event mean
// N(0, 1.2) clipped to +-5, stdv |N(0.25, 0.15)|, both rounded to 3 decimals, length ~ Geometric(0.12)), generated on the device: one
// thread per (window, row), a counter-based hash as the random source (reproducible: the same windows on every box)
namespace calib {
__device__ __forceinline__ uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float unit(uint64_t h) { return ((float)(h >> 41) + 0.5f) * (1.0f / 8388608.0f); }      // (0, 1): 23 bits + 1/2, exact in fp32
// wide = 0: the configs[1] distribution.  wide = 1 / 2 (all windows / every second window of a batch - the gate's draw since round 6; round 5 alternated
// whole batches, so a call of one batch never saw it): READ-SHAPED tails the nominal draw hardly ever produces - event
// means uniform over the whole clip range with 6 % exactly on the clip (+-5: the MAD-normalised signal is clipped there), standard deviations
// up to 9x, event lengths log-uniform from 1 to 30,000 samples (stalled events) - so that the gate sees the inputs a real run can feed
__global__ void windows_kernel(float* __restrict__ x, long long n_rows, uint64_t seed, int wide) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const uint64_t h0 = mix(seed * 0x100000001B3ull + (uint64_t)i * 4u), h1 = mix(h0), h2 = mix(h1), h3 = mix(h2);
    float* r = x + i * DM_NFEAT;
    const float uc = unit(h0);
    const int cat = uc < 0.96f ? (int)(uc * (1.0f / 0.24f)) : 4;
#pragma unroll
    for (int b = 0; b < 4; ++b) r[b] = cat == b ? 1.0f : 0.0f;
    const float rad = sqrtf(-2.0f * logf(unit(h1))), ang = 6.2831853f * unit(h2);
    const float z0 = rad * cosf(ang), z1 = rad * sinf(ang);
    r[4] = rintf(fminf(fmaxf(1.2f * z0, -5.0f), 5.0f) * 1000.0f) * 0.001f;
    r[5] = rintf(fabsf(0.25f + 0.15f * z1) * 1000.0f) * 0.001f;
    r[6] = 1.0f + floorf(logf(unit(h3)) * (1.0f / -0.12783337f));      // ln(1 - 0.12)
    if (wide == 2 ? int((i / DM_WINDOW) & 1) : wide) {        // 2: every second WINDOW of the batch (a call of a single batch sees both draws)
        const uint64_t h4 = mix(h3), h5 = mix(h4);
        const float u = unit(h4), v = unit(h5);
        r[4] = u < 0.03f ? -5.0f : (u > 0.97f ? 5.0f : rintf((10.0f * unit(h1) - 5.0f) * 1000.0f) * 0.001f);
        r[5] = rintf(fabsf(0.25f + 0.15f * z1) * (1.0f + 8.0f * v * v) * 1000.0f) * 0.001f;
        r[6] = floorf(exp2f(unit(h3) * 14.8727f));                     // 1 .. 30,000
    }
}
// largest |a - b| of two probability arrays (non-negative floats order like their bit patterns)
__global__ void maxdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n, unsigned* __restrict__ out) {
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float d = fabsf(a[i] - b[i]);
        m = (d > m || d != d) ? (d != d ? INFINITY : d) : m;
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));
}
}  // namespace calib

int dm_model_calibrate_i8(dm_model* m, int64_t n_windows, double bound, double* max_abs_dp, int* selected) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (selected) *selected = 0;
    if (max_abs_dp) *max_abs_dp = INFINITY;
    if (n_windows <= 0 || !(bound > 0.0)) return fail(DM_EINVAL, "dm_model_calibrate_i8: n_windows %lld, bound %g", (long long)n_windows, bound);
    if (!m->f16_ok) return DM_OK;                       // the split-f16 kernels are not available to this model: nothing to select
    HIP_TRY(hipSetDevice(m->device));
    int rc = sync_and_check(m);
    if (rc) return rc;
    const int64_t B = 65536;
    enum { X, PA, PB, MAX, N_TMP };
    CallBufs<N_TMP> tmp{{"dm_model_calibrate_i8"}, m->stream};
    rc = tmp.b.ensure(X, sizeof(float) * size_t(B) * DM_WINDOW * DM_NFEAT);
    if (rc == DM_OK) rc = tmp.b.ensure(PA, sizeof(float) * 2 * size_t(B));
    if (rc == DM_OK) rc = tmp.b.ensure(PB, sizeof(float) * 2 * size_t(B));
    if (rc == DM_OK) rc = tmp.b.ensure(MAX, sizeof(unsigned));
    if (rc) return rc;
    float *d_x = tmp.b.ptr<float>(X), *d_pa = tmp.b.ptr<float>(PA), *d_pb = tmp.b.ptr<float>(PB);
    unsigned* d_max = tmp.b.ptr<unsigned>(MAX);
    tmp.in_use = true;      // from here on a return waits for the stream before the temporaries go
    HIP_TRY(hipMemsetAsync(d_max, 0, sizeof(unsigned), m->stream));
    const int keep_precision = m->precision;
    const bool keep_profile = m->profile;
    m->profile = false;
    for (int64_t done = 0, batch = 0; done < n_windows && rc == DM_OK; done += B, ++batch) {
        const int64_t n = std::min<int64_t>(B, n_windows - done);
        const long long rows = (long long)n * DM_WINDOW;
        hipLaunchKernelGGL(calib::windows_kernel, dim3(unsigned((rows + 255) / 256)), dim3(256), 0, m->stream, d_x, rows, uint64_t(0x5EEDC0DEull + batch), 2);
        m->precision = DM_PREC_F32;
        rc = launch_bilstm(m, d_x, (long long)DM_WINDOW * DM_NFEAT, n, d_pa, nullptr);
        m->precision = DM_PREC_F16I8;
        if (rc == DM_OK) rc = launch_bilstm(m, d_x, (long long)DM_WINDOW * DM_NFEAT, n, d_pb, nullptr);
        if (rc == DM_OK) hipLaunchKernelGGL(calib::maxdiff_kernel, dim3(256), dim3(256), 0, m->stream, d_pa, d_pb, (long long)n * 2, d_max);
    }
    m->precision = keep_precision;
    m->profile = keep_profile;
    if (rc) return rc;                                      // (precision and profile are the caller's again on every way out)
    rc = sync_and_check(m);
    tmp.in_use = false;
    if (rc) return rc;
    unsigned bits = 0x7F800000u;
    HIP_TRY(hipMemcpy(&bits, d_max, sizeof(unsigned), hipMemcpyDeviceToHost));
    float err;
    std::memcpy(&err, &bits, 4);
    if (max_abs_dp) *max_abs_dp = double(err);
    if (double(err) <= bound && m->precision == DM_PREC_F16X3) {
        m->precision = DM_PREC_F16I8;
        m->i8_calibrated = true;
    }
    if (selected) *selected = m->precision == DM_PREC_F16I8 ? 1 : 0;      // the mode the model runs after the call
    if (m->precision != DM_PREC_F16I8) {                    // a refused model does not keep the int8 weight packs (1.7 MB)
        m->fixed.drop(dm_model::PACK0 + dm_model::PACK_SI);
        m->fixed.drop(dm_model::PACK0 + dm_model::PACK_QI);
    }
    return DM_OK;
}

// device form of a raw batch (dm_rows_emit_device) -> feature rows [n_rows][7] on the device, queued on the model's stream
int dm_rows_assemble(dm_model* m, float* d_rows, const uint8_t* d_code, const float* d_ev3, const int64_t* d_rdesc, int64_t n_reads, int64_t n_rows) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (n_rows <= 0) return DM_OK;
    if (!d_rows || !d_code || !d_ev3 || !d_rdesc || n_reads <= 0 || n_reads > 0x7fffffffLL) return fail(DM_EINVAL, "dm_rows_assemble: null array or no read");
    HIP_TRY(hipSetDevice(m->device));
    hipLaunchKernelGGL(rows_assemble_kernel, dim3(unsigned((n_rows + 255) / 256)), dim3(256), 0, m->stream, d_rows, d_code, d_ev3,
                       reinterpret_cast<const long long*>(d_rdesc), int(n_reads), (long long)n_rows);
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

int dm_model_sync(dm_model* m) {
    if (!m) return fail(DM_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    return sync_and_check(m);
}

int dm_model_get_info(dm_model* m, int key, int64_t* value) {
    if (!m || !value) return fail(DM_EINVAL, "null argument");
    switch (key) {
        case DM_INFO_PRECISION: *value = m->precision; return DM_OK;
        case DM_INFO_F16_REPRESENTABLE: *value = m->f16_ok ? 1 : 0; return DM_OK;
        case DM_INFO_F16_LENGTH_SHIFT: *value = m->len_shift; return DM_OK;
        case DM_INFO_DEVICE: *value = m->device; return DM_OK;
        case DM_INFO_GRID_CAP: *value = m->grid_cap; return DM_OK;
        case DM_INFO_LAST_GRID: *value = m->last_grid; return DM_OK;
        case DM_INFO_HAS_F16S:
#ifdef DM_WITH_F16S
            *value = 1;
#else
            *value = 0;
#endif
            return DM_OK;
        case DM_INFO_HAS_F16X3_ROLES:
#ifdef DM_WITH_F16X3_ROLES
            *value = 1;
#else
            *value = 0;
#endif
            return DM_OK;
        default: return fail(DM_EINVAL, "unknown info key %d", key);
    }
}

int dm_profile_reset(dm_model* m) {
    if (!m) return fail(DM_EINVAL, "null model");
    HIP_TRY(hipStreamSynchronize(m->stream));
    m->events_used = 0;
    m->prof_ms = 0.0;
    m->prof_launches = 0;
    m->prof_windows = 0;
    return DM_OK;
}

int dm_profile_get(dm_model* m, double* kernel_ms, int64_t* launches, int64_t* windows) {
    if (!m) return fail(DM_EINVAL, "null model");
    HIP_TRY(hipStreamSynchronize(m->stream));
    int rc = flush_profile(m);
    if (rc) return rc;
    if (kernel_ms) *kernel_ms = m->prof_ms;
    if (launches) *launches = m->prof_launches;
    if (windows) *windows = m->prof_windows;
    return DM_OK;
}

void* dm_device_alloc(int device, size_t bytes) {
    void* p = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        fail(DM_ENOMEM, "hipMalloc(%zu) on device %d failed", bytes, device);
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

int dm_device_free(int device, void* p) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(p));
    return DM_OK;
}

int dm_memcpy_h2d(int device, void* dst, const void* src, size_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return DM_OK;
}

// host -> device copy queued on the model's stream, i.e. ordered with its launches: a staging buffer can be refilled for
// the next batch without a host-side wait.  `src` must stay valid until the next dm_model_sync.
int dm_model_h2d_async(dm_model* m, void* dst, const void* src, size_t bytes) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (bytes == 0) return DM_OK;
    if (!dst || !src) return fail(DM_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, m->stream));
    return DM_OK;
}

// host -> device copy on the model's COPY stream: it does not wait for the launches already queued (it overlaps them), and
// every launch queued after this call waits for it.  The caller guarantees that nothing queued touches dst (a marker passed).
int dm_model_h2d_ahead(dm_model* m, void* dst, const void* src, size_t bytes) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (bytes == 0) return DM_OK;
    if (!dst || !src) return fail(DM_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(m->device));
    int rc = ensure_copy_stream(m);
    if (rc) return rc;
    hipEvent_t& ev = m->ahead_event[m->ahead_next];
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    m->ahead_next = (m->ahead_next + 1) % dm_model::AHEAD_EVENTS;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, m->copy_stream));
    HIP_TRY(hipEventRecord(ev, m->copy_stream));
    HIP_TRY(hipStreamWaitEvent(m->stream, ev, 0));
    return DM_OK;
}

void* dm_host_alloc(int device, size_t bytes) {
    if (hipSetDevice(device) != hipSuccess) {
        fail(DM_EDEVICE, "hipSetDevice(%d) failed", device);
        return nullptr;
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(DM_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

int dm_host_free(int device, void* p) {
    if (!p) return DM_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipHostFree(p));
    return DM_OK;
}

int dm_model_mark(dm_model* m, int i) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (i < 0 || i >= DM_MARKS) return fail(DM_EINVAL, "marker %d outside [0, %d)", i, DM_MARKS);
    HIP_TRY(hipSetDevice(m->device));
    if (!m->marks[i]) HIP_TRY(hipEventCreateWithFlags(&m->marks[i], hipEventDisableTiming));
    HIP_TRY(hipEventRecord(m->marks[i], m->stream));
    m->range.record(i);
    return DM_OK;
}

int dm_model_wait_mark(dm_model* m, int i) {
    if (!m) return fail(DM_EINVAL, "null model");
    if (i < 0 || i >= DM_MARKS) return fail(DM_EINVAL, "marker %d outside [0, %d)", i, DM_MARKS);
    if (!m->marks[i]) return DM_OK;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipEventSynchronize(m->marks[i]));
    return m->range.take_mark(i) ? range_error(m) : DM_OK;
}

int dm_memcpy_d2h(int device, void* dst, const void* src, size_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return DM_OK;
}

}  // extern "C"
