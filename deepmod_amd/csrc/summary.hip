// summary.hip — libdeepmod_hip.so, the unit behind the classifier: the per-position counters (dm_summary), their merge over ranks (the lazy RCCL
// binding, dm_comm), the CpG-cluster model (dm_cluster) and its site stage, the BED formatter.  Interface to the other units: host.h.
#include "host.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {

// ---------------------------------------------------------------------------------------------
// summary kernel: dense int32 counters with a wavefront-level pre-reduction.
// Bases arrive read by read, so a wave mostly sees 64 consecutive distinct positions (one atomic per
// counter per base), but deep pile-ups (amplicons, the cov > 1000 case of the BED format) put long
// runs of the SAME position next to each other: adjacent lanes holding the same position form a run,
// the run's head lane counts the run's flags with ballot + popcount and issues ONE atomic per
// counter for the whole run.  Integer adds commute, so the result is bit-identical either way.
// HBM-bound in principle (10 B per base in); at today's batch sizes it is launch-latency bound.
// ---------------------------------------------------------------------------------------------
__global__ void summary_add_kernel(int* __restrict__ touch, int* __restrict__ cov, int* __restrict__ mod,
                                   const long long length, const long long* __restrict__ pos,
                                   const unsigned char* __restrict__ flags,
                                   const unsigned char* __restrict__ cls, const long long n,
                                   int* __restrict__ oob) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    // whole waves iterate together so that ballots see all 64 lanes
    for (long long base = blockIdx.x * (long long)blockDim.x + (threadIdx.x & ~63); base < n; base += stride) {
        const long long i = base + lane;
        unsigned f = 0;
        long long q = -1 - lane;                      // inactive lanes get distinct keys: never merged
        if (i < n) {
            f = flags[i];
            if (cls) f = (f & 3u) | (cls[i] == 1 ? 4u : 0u);
            if (f & 1u) {
                q = pos[i];
                if (q < 0 || q >= length) {
                    atomicAdd(oob, 1);
                    f = 0;
                    q = -1 - lane;
                }
            } else {
                f = 0;
            }
        }
        const long long qprev = __shfl_up(q, 1, 64);
        const bool head = lane == 0 || q != qprev;
        const unsigned long long heads = __ballot(head);
        const unsigned long long m_touch = __ballot((f & 1u) != 0);
        const unsigned long long m_cov = __ballot((f & 3u) == 3u);
        const unsigned long long m_mod = __ballot((f & 7u) == 7u);
        if (head && (f & 1u)) {
            // run = [lane, next head)
            const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
            const int len = above ? __ffsll((long long)above) : 64 - lane;
            const unsigned long long run = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
            atomicAdd(touch + q, __popcll(m_touch & run));
            const int nc = __popcll(m_cov & run);
            if (nc) atomicAdd(cov + q, nc);
            const int nm = __popcll(m_mod & run);
            if (nm) atomicAdd(mod + q, nm);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// CpG-cluster MLP (hm_cluster_predict.py:94-103): one row per thread, weights broadcast from LDS,
// k-ascending fp32 accumulation.  60 B in/out per row, 3,420 FMA per row: VALU-bound, tiny.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cluster_mlp_kernel(const float* __restrict__ w, const float* __restrict__ x,
                                                          const long long n, float* __restrict__ out) {
    __shared__ float lw[DM_CLUSTER_WEIGHT_FLOATS];
    for (int i = threadIdx.x; i < DM_CLUSTER_WEIGHT_FLOATS; i += blockDim.x) lw[i] = w[i];
    __syncthreads();
    const float* W1 = lw;             // [14][100]
    const float* b1 = lw + 1400;      // [100]
    const float* W2 = lw + 1500;      // [100][20]
    const float* b2 = lw + 3500;      // [20]
    const float* WO = lw + 3520;      // [20]
    const float bO = lw[3540];
    for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        float xi[14];
#pragma unroll
        for (int k = 0; k < 14; ++k) xi[k] = x[r * 14 + k];
        float h2[20];
#pragma unroll
        for (int j = 0; j < 20; ++j) h2[j] = 0.0f;
        for (int u = 0; u < 100; ++u) {
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k < 14; ++k) a = fmaf(xi[k], W1[k * 100 + u], a);
            a = fmaxf(a + b1[u], 0.0f);                 // layer_1 = relu(X W_1 + b_1); dropout(keep_prob 1) = identity
#pragma unroll
            for (int j = 0; j < 20; ++j) h2[j] = fmaf(a, W2[u * 20 + j], h2[j]);
        }
        float o = 0.0f;
#pragma unroll
        for (int j = 0; j < 20; ++j) o = fmaf(fmaxf(h2[j] + b2[j], 0.0f), WO[j], o);   // layer_2 = relu(.), then W_O
        o += bO;
        out[r] = 1.0f / (1.0f + expf(-o));              // output = sigmoid(.)
    }
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------- summary ----
dm_summary* dm_summary_create(int device, int64_t length) {
    if (length <= 0 || length > (int64_t(1) << 33)) {
        fail(DM_EINVAL, "bad contig length %lld", (long long)length);
        return nullptr;
    }
    dm_summary* s = new (std::nothrow) dm_summary();
    if (!s) {
        fail(DM_ENOMEM, "out of host memory");
        return nullptr;
    }
    s->device = device;
    s->length = length;
    bool ok = hipSetDevice(device) == hipSuccess &&
              hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&s->d_counts, sizeof(int) * (3 * length + dm_summary::SLACK)) == hipSuccess &&
              hipMalloc(&s->d_oob, sizeof(int)) == hipSuccess &&
              // on the summary's own (non-blocking) stream and waited for: a memset on the null stream is not ordered with the
              // kernels that the summary's or a followed model's stream run next (3 GB of counters take a millisecond to clear)
              hipMemsetAsync(s->d_counts, 0, sizeof(int) * (3 * length + dm_summary::SLACK), s->stream) == hipSuccess &&
              hipMemsetAsync(s->d_oob, 0, sizeof(int), s->stream) == hipSuccess &&
              hipStreamSynchronize(s->stream) == hipSuccess;
    if (!ok) {
        fail(DM_EDEVICE, "summary allocation of %lld positions on device %d failed: %s", (long long)length, device,
             hipGetErrorString(hipGetLastError()));
        dm_summary_destroy(s);
        return nullptr;
    }
    return s;
}

void dm_summary_destroy(dm_summary* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipFree(s->d_counts);
    (void)hipFree(s->d_oob);
    s->b.release();
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int64_t dm_summary_length(const dm_summary* s) { return s ? s->length : 0; }

static int summary_add_impl(dm_summary* s, const int64_t* pos, const uint8_t* flags, const uint8_t* cls, int64_t n,
                            bool* deferred = nullptr) {
    if (!s) return fail(DM_EINVAL, "null summary");
    if (n < 0) return fail(DM_EINVAL, "negative count");
    if (n == 0) return DM_OK;
    if (!pos || !flags) return fail(DM_EINVAL, "null input");
    HIP_TRY(hipSetDevice(s->device));
    const long long* dpos = reinterpret_cast<const long long*>(pos);
    const unsigned char* dfl = flags;
    const unsigned char* dcl = cls;
    const bool pd = is_device_ptr(pos), fd = is_device_ptr(flags), cd = cls ? is_device_ptr(cls) : true;
    if (!(pd && fd && cd)) {
        const size_t room = size_t(std::max<int64_t>(n, dm_summary::STAGE_FLOOR));     // small adds never regrow the pair
        int rc;
        if ((rc = s->b.ensure(dm_summary::POS, sizeof(long long) * room)) != DM_OK || (rc = s->b.ensure(dm_summary::FLAGS, 2 * room)) != DM_OK) return rc;
        long long* d_pos = s->b.ptr<long long>(dm_summary::POS);
        unsigned char* d_flags = s->b.ptr<unsigned char>(dm_summary::FLAGS);     // flags [n] | cls [n]
        if (!pd) {
            HIP_TRY(hipMemcpyAsync(d_pos, pos, sizeof(long long) * n, hipMemcpyHostToDevice, s->stream));
            dpos = d_pos;
        }
        if (!fd) {
            HIP_TRY(hipMemcpyAsync(d_flags, flags, n, hipMemcpyHostToDevice, s->stream));
            dfl = d_flags;
        }
        if (cls && !cd) {
            HIP_TRY(hipMemcpyAsync(d_flags + n, cls, n, hipMemcpyHostToDevice, s->stream));
            dcl = d_flags + n;
        }
    }
    const int threads = 256;
    const int blocks = int(std::min<int64_t>((n + threads - 1) / threads, 2048));
    hipStream_t st = s->stream;
    if (s->follow) {
        if (pd && fd && cd) {
            st = model_stream(s->follow);                           // device-resident inputs: one in-order queue with the classifier
            if (deferred && model_async(s->follow)) *deferred = true;     // out-of-range check waits for dm_summary_sync / fetch
        }
        else HIP_TRY(hipStreamSynchronize(model_stream(s->follow)));      // staged inputs travel on the summary's own stream
    }
    hipLaunchKernelGGL(summary_add_kernel, dim3(blocks), dim3(threads), 0, st, s->d_counts,
                       s->d_counts + s->length, s->d_counts + 2 * s->length, (long long)s->length, dpos, dfl, dcl,
                       (long long)n, s->d_oob);
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

static int summary_check_oob(dm_summary* s) {
    int oob = 0;
    if (s->follow) HIP_TRY(hipStreamSynchronize(model_stream(s->follow)));
    HIP_TRY(hipMemcpyAsync(&oob, s->d_oob, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (oob) {
        HIP_TRY(hipMemsetAsync(s->d_oob, 0, sizeof(int), s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        return fail(DM_EINVAL, "%d positions outside [0, %lld) were dropped", oob, (long long)s->length);
    }
    return DM_OK;
}

int dm_summary_add(dm_summary* s, const int64_t* pos, const uint8_t* flags, int64_t n) {
    bool deferred = false;
    int rc = summary_add_impl(s, pos, flags, nullptr, n, &deferred);
    if (rc || n <= 0 || deferred) return rc;
    return summary_check_oob(s);  // synchronous on return (the caller may reuse its buffers)
}

int dm_summary_add_classified(dm_summary* s, const int64_t* pos, const uint8_t* flags, const uint8_t* cls,
                              int64_t n) {
    if (n > 0 && !cls) return fail(DM_EINVAL, "null cls");
    bool deferred = false;
    int rc = summary_add_impl(s, pos, flags, cls, n, &deferred);
    if (rc || n <= 0 || deferred) return rc;
    return summary_check_oob(s);
}

int dm_summary_sync(dm_summary* s) {
    if (!s) return fail(DM_EINVAL, "null summary");
    HIP_TRY(hipSetDevice(s->device));
    return summary_check_oob(s);
}

int dm_summary_fetch(dm_summary* s, int32_t* touch, int32_t* cov, int32_t* mod) {
    if (!s) return fail(DM_EINVAL, "null summary");
    HIP_TRY(hipSetDevice(s->device));
    int rc0 = summary_check_oob(s);
    if (rc0) return rc0;
    const size_t bytes = sizeof(int) * s->length;
    if (touch) HIP_TRY(hipMemcpy(touch, s->d_counts, bytes, hipMemcpyDeviceToHost));
    if (cov) HIP_TRY(hipMemcpy(cov, s->d_counts + s->length, bytes, hipMemcpyDeviceToHost));
    if (mod) HIP_TRY(hipMemcpy(mod, s->d_counts + 2 * s->length, bytes, hipMemcpyDeviceToHost));
    return DM_OK;
}

void* dm_summary_device_ptr(dm_summary* s) { return s ? s->d_counts : nullptr; }

int dm_summary_follow(dm_summary* s, dm_model* m) {
    if (!s) return fail(DM_EINVAL, "null summary");
    if (m && model_device(m) != s->device) return fail(DM_EINVAL, "summary (device %d) cannot follow a model on device %d", s->device, model_device(m));
    if (s->follow) HIP_TRY(hipStreamSynchronize(model_stream(s->follow)));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->follow = m;
    return DM_OK;
}

// ------------------------------------------------------------------------------- cluster ----
dm_cluster* dm_cluster_create(int device, const float* weights, size_t n_floats) {
    if (!weights || n_floats != DM_CLUSTER_WEIGHT_FLOATS) {
        fail(DM_EINVAL, "cluster weights: expected %d floats, got %zu", DM_CLUSTER_WEIGHT_FLOATS, n_floats);
        return nullptr;
    }
    dm_cluster* c = new (std::nothrow) dm_cluster();
    if (!c) {
        fail(DM_ENOMEM, "out of host memory");
        return nullptr;
    }
    c->device = device;
    bool ok = hipSetDevice(device) == hipSuccess &&
              hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&c->d_w, sizeof(float) * n_floats) == hipSuccess &&
              hipMemcpy(c->d_w, weights, sizeof(float) * n_floats, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        fail(DM_EDEVICE, "cluster model setup on device %d failed: %s", device, hipGetErrorString(hipGetLastError()));
        dm_cluster_destroy(c);
        return nullptr;
    }
    return c;
}

void dm_cluster_destroy(dm_cluster* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipFree(c->d_w);
    c->stage.release();
    c->sites.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int dm_cluster_predict(dm_cluster* c, const float* x, int64_t n, float* out) {
    if (!c) return fail(DM_EINVAL, "null cluster model");
    if (n < 0) return fail(DM_EINVAL, "negative row count");
    if (n == 0) return DM_OK;
    if (!x || !out) return fail(DM_EINVAL, "null buffer");
    HIP_TRY(hipSetDevice(c->device));
    const bool xd = is_device_ptr(x), od = is_device_ptr(out);
    int rc;
    const float* dx = x;
    float* dout = out;
    if (!xd) {
        if ((rc = c->stage.ensure(dm_cluster::X, sizeof(float) * 14 * n)) != DM_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c->stage.buf[dm_cluster::X], x, sizeof(float) * 14 * n, hipMemcpyHostToDevice, c->stream));
        dx = c->stage.ptr<float>(dm_cluster::X);
    }
    if (!od) {
        if ((rc = c->stage.ensure(dm_cluster::OUT, sizeof(float) * n)) != DM_OK) return rc;
        dout = c->stage.ptr<float>(dm_cluster::OUT);
    }
    const int blocks = int(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(cluster_mlp_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_w, dx, (long long)n, dout);
    HIP_TRY(hipGetLastError());
    if (!od) HIP_TRY(hipMemcpyAsync(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return DM_OK;
}

// ---- RCCL, loaded lazily so single-GPU users never need it ---------------------------------
namespace {
// The library is found with dlopen (a one-GPU user never needs it, and DEEPMOD_RCCL_LIBRARY may name a site build), but every type, enumerator and
// prototype is RCCL's own, from <rccl/rccl.h>: a drift between what is called here and what the library exports is a compile error in this file -
// and in tests/shim/shmccl.cpp, which defines the same functions against the same header - not a surprise on the first eight-rank run.
static_assert(sizeof(ncclUniqueId) == 128 && NCCL_UNIQUE_ID_BYTES == 128, "the C ABI hands the RCCL id around as 128 bytes (dm_rccl_unique_id)");
struct Rccl {
    void* h = nullptr;
    std::string path;                                  // what dlopen was given
    int version = 0;                                   // ncclGetVersion, 0 if the library has none
    decltype(&ncclGetUniqueId) getid = nullptr;
    decltype(&ncclCommInitRank) init = nullptr;
    decltype(&ncclAllReduce) allreduce = nullptr;
    decltype(&ncclReduce) reduce = nullptr;
    decltype(&ncclReduceScatter) reducescatter = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclGetErrorString) errstr = nullptr;
    decltype(&ncclGetVersion) getversion = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;   // optional: one launch for the three counter arrays of a reduce-scatter
    decltype(&ncclGroupEnd) group_end = nullptr;
};
Rccl g_rccl;

int load_rccl() {
    if (g_rccl.h) return DM_OK;
    // DEEPMOD_RCCL_LIBRARY names the collective library to bind instead of the system's librccl (a site build of RCCL; the one-GPU test
    // transport tests/shim/shmccl.cpp).  When it is set nothing else is tried: a wrong path is an error, not a silent fall back.
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    const char* named = std::getenv("DEEPMOD_RCCL_LIBRARY");
    if (named && *named) {
        h = dlopen(named, RTLD_NOW | RTLD_LOCAL);
        if (!h) return fail(DM_ERCCL, "cannot dlopen DEEPMOD_RCCL_LIBRARY=%s: %s", named, dlerror());
        g_rccl.path = named;
    }
    for (const char* nm : names) {
        if (h) break;
        h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
        if (h) g_rccl.path = nm;
    }
    if (!h) return fail(DM_ERCCL, "cannot dlopen librccl: %s", dlerror());
    auto bind = [h](const char* name, auto& fn) { fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name)); };
    bind("ncclGetUniqueId", g_rccl.getid);
    bind("ncclCommInitRank", g_rccl.init);
    bind("ncclAllReduce", g_rccl.allreduce);
    bind("ncclReduce", g_rccl.reduce);
    bind("ncclReduceScatter", g_rccl.reducescatter);
    bind("ncclCommDestroy", g_rccl.destroy);
    bind("ncclGetErrorString", g_rccl.errstr);
    bind("ncclGetVersion", g_rccl.getversion);
    bind("ncclGroupStart", g_rccl.group_start);
    bind("ncclGroupEnd", g_rccl.group_end);
    if (!g_rccl.getid || !g_rccl.init || !g_rccl.allreduce || !g_rccl.reduce || !g_rccl.destroy)
        return fail(DM_ERCCL, "librccl is missing required symbols");
    if (g_rccl.getversion && g_rccl.getversion(&g_rccl.version) != ncclSuccess) g_rccl.version = 0;
    {   // the file the loader really mapped (librccl.so.1 -> /opt/rocm-7.2.0/lib/librccl.so.1.0...): what a run's log should name
        Dl_info info;
        if (dladdr(reinterpret_cast<void*>(g_rccl.getid), &info) && info.dli_fname && *info.dli_fname) g_rccl.path = info.dli_fname;
    }
    g_rccl.h = h;
    return DM_OK;
}
const char* rccl_err(ncclResult_t e) { return g_rccl.errstr ? g_rccl.errstr(e) : "error"; }
}  // namespace

struct dm_comm {
    int device = 0, rank = 0, nranks = 1;
    ncclComm_t comm = nullptr;
    hipStream_t stream = nullptr;
    double* d_scalar = nullptr;    // one device double for barrier / max
    int64_t reduces = 0;           // collectives issued (dm_comm_stats)
    int64_t reduced_bytes = 0;
};

// Which collective library this process bound (loading it if that has not happened yet): the file the loader mapped and ncclGetVersion's code
// (e.g. 22207 = 2.22.7; 0 if the library has no such entry).  What `detect --gpus N` prints at the start of a multi-GPU run.
int dm_rccl_info(char* path, int path_len, int* version) {
    int rc = load_rccl();
    if (rc) return rc;
    if (path && path_len > 0) {
        std::strncpy(path, g_rccl.path.c_str(), size_t(path_len) - 1);
        path[path_len - 1] = 0;
    }
    if (version) *version = g_rccl.version;
    return DM_OK;
}

int dm_rccl_unique_id(void* out128) {
    if (!out128) return fail(DM_EINVAL, "null id buffer");
    int rc = load_rccl();
    if (rc) return rc;
    ncclUniqueId id;
    ncclResult_t e = g_rccl.getid(&id);
    if (e != ncclSuccess) return fail(DM_ERCCL, "ncclGetUniqueId: %s", rccl_err(e));
    std::memcpy(out128, &id, 128);
    return DM_OK;
}

dm_comm* dm_comm_create(int device, const void* unique_id128, int rank, int nranks) {
    if (!unique_id128 || nranks < 1 || rank < 0 || rank >= nranks) {
        fail(DM_EINVAL, "bad communicator arguments (rank %d of %d)", rank, nranks);
        return nullptr;
    }
    if (load_rccl() != DM_OK) return nullptr;
    dm_comm* c = new (std::nothrow) dm_comm();
    if (!c) {
        fail(DM_ENOMEM, "out of host memory");
        return nullptr;
    }
    c->device = device;
    c->rank = rank;
    c->nranks = nranks;
    ncclUniqueId id;
    std::memcpy(&id, unique_id128, 128);
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&c->d_scalar, sizeof(double)) == hipSuccess;
    if (!ok) {
        fail(DM_EDEVICE, "communicator setup on device %d failed: %s", device, hipGetErrorString(hipGetLastError()));
        dm_comm_destroy(c);
        return nullptr;
    }
    ncclResult_t e = g_rccl.init(&c->comm, nranks, id, rank);       // collective over all ranks: every rank calls it once
    if (e != ncclSuccess) {
        fail(DM_ERCCL, "ncclCommInitRank(rank %d of %d): %s", rank, nranks, rccl_err(e));
        c->comm = nullptr;
        dm_comm_destroy(c);
        return nullptr;
    }
    return c;
}

void dm_comm_destroy(dm_comm* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm) g_rccl.destroy(c->comm);
    (void)hipFree(c->d_scalar);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int dm_comm_rank(const dm_comm* c) { return c ? c->rank : -1; }
int dm_comm_size(const dm_comm* c) { return c ? c->nranks : 0; }

int dm_comm_stats(const dm_comm* c, int64_t* collectives, int64_t* bytes) {
    if (!c) return fail(DM_EINVAL, "null communicator");
    if (collectives) *collectives = c->reduces;
    if (bytes) *bytes = c->reduced_bytes;
    return DM_OK;
}

// max over ranks of *value (in place); with value == NULL a plain barrier.  Host-synchronous.
int dm_comm_max_f64(dm_comm* c, double* value) {
    if (!c) return fail(DM_EINVAL, "null communicator");
    HIP_TRY(hipSetDevice(c->device));
    double v = value ? *value : 0.0;
    HIP_TRY(hipMemcpyAsync(c->d_scalar, &v, sizeof v, hipMemcpyHostToDevice, c->stream));
    ncclResult_t e = g_rccl.allreduce(c->d_scalar, c->d_scalar, 1, ncclFloat64, ncclMax, c->comm, c->stream);
    if (e != ncclSuccess) return fail(DM_ERCCL, "ncclAllReduce(max): %s", rccl_err(e));
    HIP_TRY(hipMemcpyAsync(&v, c->d_scalar, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (value) *value = v;
    return DM_OK;
}
int dm_comm_barrier(dm_comm* c) { return dm_comm_max_f64(c, nullptr); }

// In-place sum of touch|cov|mod over the ranks of `c` (int32, order independent -> the BED is the same for any sharding):
// root >= 0: ncclReduce, the result is valid on `root` only (what the final per-position summary needs);
// root < 0 : ncclAllReduce, valid everywhere.  All ranks must call it for summaries of the same length, in the same order.
int dm_summary_reduce(dm_summary* s, dm_comm* c, int root) {
    if (!s || !c) return fail(DM_EINVAL, "null summary / communicator");
    if (root >= c->nranks) return fail(DM_EINVAL, "root %d outside the %d ranks", root, c->nranks);
    if (s->device != c->device) return fail(DM_EINVAL, "summary on device %d, communicator on device %d", s->device, c->device);
    HIP_TRY(hipSetDevice(s->device));
    if (s->follow) HIP_TRY(hipStreamSynchronize(model_stream(s->follow)));   // adds queued on the classifier's stream
    HIP_TRY(hipStreamSynchronize(s->stream));
    const size_t count = size_t(3) * s->length;
    ncclResult_t e = root >= 0 ? g_rccl.reduce(s->d_counts, s->d_counts, count, ncclInt32, ncclSum, root, c->comm, c->stream)
                      : g_rccl.allreduce(s->d_counts, s->d_counts, count, ncclInt32, ncclSum, c->comm, c->stream);
    if (e != ncclSuccess) return fail(DM_ERCCL, "%s: %s", root >= 0 ? "ncclReduce" : "ncclAllReduce", rccl_err(e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->reduces;
    c->reduced_bytes += int64_t(count) * 4;
    return DM_OK;
}

// Grow the counters to `new_length` positions (new positions zero).  A worker that learns contig lengths from its reads
// sizes the counters as it goes; before a reduce all ranks grow to the common length.
int dm_summary_grow(dm_summary* s, int64_t new_length) {
    if (!s) return fail(DM_EINVAL, "null summary");
    if (new_length <= s->length) return DM_OK;
    if (new_length > (int64_t(1) << 33)) return fail(DM_EINVAL, "bad contig length %lld", (long long)new_length);
    HIP_TRY(hipSetDevice(s->device));
    if (s->follow) HIP_TRY(hipStreamSynchronize(model_stream(s->follow)));
    HIP_TRY(hipStreamSynchronize(s->stream));
    int* nd = nullptr;
    if (hipMalloc(&nd, sizeof(int) * (3 * new_length + dm_summary::SLACK)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DM_ENOMEM, "cannot grow the summary to %lld positions", (long long)new_length);
    }
    hipError_t e = hipMemsetAsync(nd, 0, sizeof(int) * (3 * new_length + dm_summary::SLACK), s->stream);
    for (int k = 0; k < 3 && e == hipSuccess; ++k)
        e = hipMemcpyAsync(nd + k * new_length, s->d_counts + k * s->length, sizeof(int) * s->length, hipMemcpyDeviceToDevice, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        (void)hipFree(nd);                         // the old counters stay valid
        return fail(DM_EDEVICE, "growing the summary to %lld positions failed: %s", (long long)new_length, hipGetErrorString(e));
    }
    HIP_TRY(hipFree(s->d_counts));
    s->d_counts = nd;
    s->length = new_length;
    s->slice_count = -1;
    return DM_OK;
}

// Scatter form of the merge: positions are cut into nranks slices of chunk = ceil(length / nranks); after the call
// rank r holds the sums over all ranks of touch | cov | mod for its slice [r * chunk, min(length, (r + 1) * chunk)) and formats
// that part of the BED itself - no rank fetches or formats a whole contig.  One ncclReduceScatter per counter array (int32 sum).
int dm_summary_reduce_scatter(dm_summary* s, dm_comm* c, int64_t* first, int64_t* count) {
    if (!s || !c) return fail(DM_EINVAL, "null summary / communicator");
    if (s->device != c->device) return fail(DM_EINVAL, "summary on device %d, communicator on device %d", s->device, c->device);
    if (c->nranks > dm_summary::SLACK) return fail(DM_EINVAL, "reduce-scatter over %d ranks (at most %lld)", c->nranks, (long long)dm_summary::SLACK);
    if (!g_rccl.reducescatter) return fail(DM_ERCCL, "librccl has no ncclReduceScatter");
    HIP_TRY(hipSetDevice(s->device));
    if (s->follow) HIP_TRY(hipStreamSynchronize(model_stream(s->follow)));   // adds queued on the classifier's stream
    HIP_TRY(hipStreamSynchronize(s->stream));
    const int64_t chunk = (s->length + c->nranks - 1) / c->nranks;
    s->slice_count = -1;                              // whatever the block held is gone from here on
    const int rcb = s->b.ensure(dm_summary::SLICE, sizeof(int) * 3 * size_t(chunk));
    if (rcb != DM_OK) return rcb;
    s->slice_chunk = chunk;
    // the three counter arrays as ONE group where librccl has the group calls (one fused launch per rank instead of three)
    const bool grouped = g_rccl.group_start && g_rccl.group_end;
    if (grouped) {
        ncclResult_t e = g_rccl.group_start();
        if (e != ncclSuccess) return fail(DM_ERCCL, "ncclGroupStart: %s", rccl_err(e));
    }
    ncclResult_t err = ncclSuccess;
    for (int k = 0; k < 3 && err == ncclSuccess; ++k) {
        // the send buffer of array k is read up to nranks * chunk <= length + nranks - 1 positions: past `length` that is the head of
        // the next array (or the allocation's slack) - sums of positions that do not exist, never looked at
        err = g_rccl.reducescatter(s->d_counts + k * s->length, s->slice() + k * s->slice_chunk, size_t(chunk), ncclInt32, ncclSum, c->comm, c->stream);
    }
    if (grouped) {
        const ncclResult_t e = g_rccl.group_end();     // always closed, also after a failed call inside the group
        if (err == ncclSuccess) err = e;
    }
    if (err != ncclSuccess) return fail(DM_ERCCL, "ncclReduceScatter: %s", rccl_err(err));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->reduces;
    c->reduced_bytes += int64_t(3) * s->length * 4;
    s->slice_first = std::min<int64_t>(s->length, int64_t(c->rank) * chunk);
    s->slice_count = std::min<int64_t>(s->length, int64_t(c->rank + 1) * chunk) - s->slice_first;
    if (first) *first = s->slice_first;
    if (count) *count = s->slice_count;
    return DM_OK;
}

// this rank's slice after dm_summary_reduce_scatter: `count` int32 each (any may be NULL)
int dm_summary_fetch_slice(dm_summary* s, int32_t* touch, int32_t* cov, int32_t* mod) {
    if (!s) return fail(DM_EINVAL, "null summary");
    if (s->slice_count < 0) return fail(DM_ESTATE, "no reduce-scatter result: call dm_summary_reduce_scatter first");
    HIP_TRY(hipSetDevice(s->device));
    int rc0 = summary_check_oob(s);
    if (rc0) return rc0;
    const size_t bytes = sizeof(int) * size_t(s->slice_count);
    if (bytes == 0) return DM_OK;
    if (touch) HIP_TRY(hipMemcpy(touch, s->slice(), bytes, hipMemcpyDeviceToHost));
    if (cov) HIP_TRY(hipMemcpy(cov, s->slice() + s->slice_chunk, bytes, hipMemcpyDeviceToHost));
    if (mod) HIP_TRY(hipMemcpy(mod, s->slice() + 2 * s->slice_chunk, bytes, hipMemcpyDeviceToHost));
    return DM_OK;
}

}  // extern "C"

#include "bedtext.inc"
#include "cluster_sites.hip.inc"
