// cluster_train.hip.inc — training of the CpG-cluster MLP for gfx950 (part of offline.hip): forward, backward, Adam.
//
// The network is the reference's serialized training graph (train_deepmod/na12878_cluster_train_mod-keep_prob0.7-nb25-chr1/Cg.cov5.nb25.meta):
//   layer_1 = relu(X W_1 + b_1), d_1 = layer_1 / keep_prob * floor(keep_prob + U[0,1));  layer_2 = relu(d_1 W_2 + b_2), d_2 the same;
//   output = sigmoid(d_2 W_O + b_O);  loss = mean((output - Y)^2) over the n rows;  AdamOptimizer(0.001).
// The rules of train.hip.inc hold: fp32 throughout, plain launches on the handle's stream, no graph capture, no grid barrier, no float atomic; every
// output element has one writer and every reduction a fixed order, so two runs are bit-identical.  The weights are the canonical 3,541-float blob
// of cluster.flatten_cluster_weights (W_1 b_1 W_2 b_2 W_O b_O), which Adam updates in place.
//
//   grad_kernel     one block = one wave = 64 rows, one row per lane, weights in LDS.  The forward of a row is lane-local in the accumulation order of
//                   cluster_mlp_kernel (k ascending fmaf, bias after the sum), so at keep_prob 1 `out` is that kernel's bit for bit.  Backward per row:
//                   d_o = 2 (out - y) / n * out (1 - out), then back through W_O, mask 2, ReLU, W_2, mask 1, ReLU; layer_1 is recomputed unit by unit.
//                   dW_1 = [X | 1]^T dPre_1 ([16 x 64] [64 x 112]) and dW_2 = [d_1 | 1]^T dPre_2 ([112 x 64] [64 x 32]) are v_mfma_f32_16x16x4_f32 products
//                   with the 64 rows as K, staged through LDS 16 units at a time; the row of ones makes the bias gradients a row of the product.
//                   dW_O, db_O and the sum of squared errors are wave reductions (xor tree, fixed order).  Each block writes one partial blob.
//   reduce_kernel   the block partials summed in block order -> the gradient blob; the loss from the per-block sums in block order
//   mask_kernel     the generated dropout mask as bytes (dm_cluster_trainer_mask; the tests hold it to cluster_train.dropout_keep)
//   dmtrain::adam_kernel   as it is, on 3,541 floats
// A step is three launches (grad, reduce, adam) and no host round trip.  Its work is about 18 kFLOP and 60 B per row, but it is not launch-bound:
// a lane runs a row's whole forward and backward alone, and grad_kernel's time is that chain's latency (DESIGN 15 has the measured times).
//
// The dropout mask is this project's own (TensorFlow's random stream cannot be reproduced): a counter-based generator keyed by
// (seed, step, row in batch, pair of units), units 0..99 = layer 1, 100..119 = layer 2.  Its definition is cluster_train.dropout_keep (numpy).
#pragma once
#include "host.h"
#include "train.hip.inc"

namespace dmct {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int NIN = 14, H1 = 100, H2 = 20, NW = DM_CLUSTER_WEIGHT_FLOATS, MASKW = H1 + H2;
constexpr int OFF_B1 = 1400, OFF_W2 = 1500, OFF_B2 = 3500, OFF_WO = 3520, OFF_BO = 3540;
constexpr int ROWS = 64;                             // rows per block (one wave, one row per lane)
constexpr int UG = 7;                                // unit groups of 16 (100 units + the row of ones -> 112)
constexpr int64_t MAX_BATCH = 1 << 16;               // 1,024 partial blobs

__host__ __device__ inline uint64_t mix(uint64_t z) {           // splitmix64's finalizer
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t mask_key(uint64_t seed, uint64_t step) { return mix(mix(seed) + step); }

// One 64-bit hash serves a pair of units (the 64-bit multiplies of mix are the expensive part): unit 2p takes bits 63..41, unit 2p + 1 bits 40..18.
// keep = floor(keep_prob + u) in float32, u = 23 random bits / 2^23 in [0, 1): keep_prob + u <= 2 - 2^-23 is representable, so keep is 0 or 1.
__device__ __forceinline__ uint64_t pair_hash(const uint64_t key, const long long row, const int pair) { return mix(key + (uint64_t)row * 64u + (uint64_t)pair); }
__device__ __forceinline__ float keep_from(const uint64_t h, const int odd, const float kp) {
    const unsigned bits = odd ? (unsigned)(h >> 18) & 0x7FFFFFu : (unsigned)(h >> 41);
    return floorf(kp + (float)bits * (1.0f / 8388608.0f));
}

__device__ __forceinline__ float wave_sum(float s) {
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

// x, y: the rows themselves (ids == nullptr) or the resident data the ids index (n_src rows).  mask: [n][120] bytes or nullptr (generated from key).
__global__ __launch_bounds__(64) void grad_kernel(const float* __restrict__ w, const float* __restrict__ x, const float* __restrict__ y,
                                                  const long long* __restrict__ ids, const long long n_src, const long long n, const float kp,
                                                  const unsigned char* __restrict__ mask, const uint64_t key, float* __restrict__ out,
                                                  float* __restrict__ part, float* __restrict__ lossp) {
    __shared__ __attribute__((aligned(16))) float w1t[H1][16];   // W_1 transposed, [unit][feature | 0 0]: the 14 weights of a unit in four 16-byte reads
    __shared__ __attribute__((aligned(16))) float lw[NW - OFF_B1];                           // b_1 W_2 b_2 W_O b_O as they lie in the blob
    __shared__ float xs[ROWS][17];                   // [row][feature | 1 | 0]; 17: rows of a k-step fall into different banks
    __shared__ float a1c[ROWS][17];                  // d_1 of the 16 units of a group
    __shared__ float dp1c[ROWS][17];                 // dPre_1 of the same units
    __shared__ float dp2s[ROWS][33];                 // dPre_2, 20 -> 32 with zeros
    const int lane = threadIdx.x;
    const int col = lane & 15, quad = lane >> 4;
    // one wave brings in 14 KB: 16-byte loads, all of them in flight at once (the blob is a hipMalloc block and OFF_B1 * 4 a multiple of 16)
    const float4* w4 = reinterpret_cast<const float4*>(w);
#pragma unroll
    for (int it = 0; it < (OFF_B1 / 4 + ROWS - 1) / ROWS; ++it) {
        const int i = lane + ROWS * it;
        if (i < OFF_B1 / 4) {
            const float4 v = w4[i];
            const int k = (4 * i) / H1, u = (4 * i) % H1;           // H1 is a multiple of 4: the four values are units u .. u + 3 of feature k
            w1t[u][k] = v.x;
            w1t[u + 1][k] = v.y;
            w1t[u + 2][k] = v.z;
            w1t[u + 3][k] = v.w;
        }
    }
    for (int u = lane; u < H1; u += ROWS) w1t[u][14] = w1t[u][15] = 0.0f;
    constexpr int TAIL4 = (NW - OFF_B1) / 4;                         // 535 whole float4 and one float
#pragma unroll
    for (int it = 0; it < (TAIL4 + ROWS - 1) / ROWS; ++it) {
        const int i = lane + ROWS * it;
        if (i < TAIL4) reinterpret_cast<float4*>(lw)[i] = w4[OFF_B1 / 4 + i];
    }
    if (lane == 0) lw[4 * TAIL4] = w[OFF_B1 + 4 * TAIL4];
    static_assert(OFF_B1 % 4 == 0 && H1 % 4 == 0 && NW - OFF_B1 == 4 * TAIL4 + 1, "the 16-byte loads above");
    const float* b1 = lw;
    const float* W2 = lw + (OFF_W2 - OFF_B1);
    const float* b2 = lw + (OFF_B2 - OFF_B1);
    const float* WO = lw + (OFF_WO - OFF_B1);

    const long long r = (long long)blockIdx.x * ROWS + lane;
    bool valid = r < n;
    long long src = r;
    if (valid && ids) {
        src = ids[r];
        if (src < 0 || src >= n_src) valid = false;  // the host has refused such a batch already; never read outside the data
    }
    float xi[NIN], yv = 0.0f;
#pragma unroll
    for (int k = 0; k < NIN; ++k) xi[k] = valid ? x[src * NIN + k] : 0.0f;
    if (valid) yv = y[src];
#pragma unroll
    for (int k = 0; k < NIN; ++k) xs[lane][k] = xi[k];
    xs[lane][14] = valid ? 1.0f : 0.0f;
    xs[lane][15] = 0.0f;
    const unsigned char* mk = mask ? mask + r * MASKW : nullptr;
    __syncthreads();

    // ---- forward, lane-local
    float h2[H2];
#pragma unroll
    for (int j = 0; j < H2; ++j) h2[j] = 0.0f;
    unsigned long long keep_lo = 0, keep_hi = 0;      // the row's layer-1 mask, units 0..63 and 64..99: the backward pass reads it back
    for (int p = 0; p < H1 / 2; ++p) {
        const uint64_t h = mk ? 0 : pair_hash(key, r, p);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int u = 2 * p + q;
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k < NIN; ++k) a = fmaf(xi[k], w1t[u][k], a);
            a = fmaxf(a + b1[u], 0.0f);
            const float kf = valid ? (mk ? (float)mk[u] : keep_from(h, q, kp)) : 0.0f;
            const unsigned long long bit = kf != 0.0f ? 1ull : 0ull;
            if (u < 64) keep_lo |= bit << u;
            else keep_hi |= bit << (u - 64);
            const float d = a / kp * kf;
#pragma unroll
            for (int j = 0; j < H2; ++j) h2[j] = fmaf(d, W2[u * H2 + j], h2[j]);
        }
    }
    float d2[H2], g2[H2];                             // d_2, then dPre_2
    float o = 0.0f;
#pragma unroll
    for (int j = 0; j < H2; ++j) {
        const float pre = h2[j] + b2[j];
        const float kf = valid ? (mk ? (float)mk[H1 + j] : keep_from(pair_hash(key, r, (H1 + j) / 2), j & 1, kp)) : 0.0f;
        d2[j] = fmaxf(pre, 0.0f) / kp * kf;
        o = fmaf(d2[j], WO[j], o);
        g2[j] = pre > 0.0f ? kf : 0.0f;              // the mask where the ReLU passes; scaled by d_o W_O / keep_prob below
    }
    o += lw[OFF_BO - OFF_B1];
    const float res = 1.0f / (1.0f + expf(-o));
    if (valid && out) out[r] = res;
    const float diff = res - yv;
    const float d_o = valid ? 2.0f * diff / (float)n * (res * (1.0f - res)) : 0.0f;

    float* bp = part + (size_t)blockIdx.x * NW;
#pragma unroll
    for (int j = 0; j < H2; ++j) {
        const float s = wave_sum(d2[j] * d_o);
        if (lane == 0) bp[OFF_WO + j] = s;
        g2[j] = d_o * WO[j] * g2[j] / kp;
        dp2s[lane][j] = g2[j];
    }
#pragma unroll
    for (int j = H2; j < 32; ++j) dp2s[lane][j] = 0.0f;
    {
        const float s = wave_sum(d_o), l = wave_sum(valid ? diff * diff : 0.0f);
        if (lane == 0) {
            bp[OFF_BO] = s;
            lossp[blockIdx.x] = l;
        }
    }

    // ---- backward through layer 1, 16 units at a time: lane-local dPre_1, then the two products over the 64 rows
    for (int g = 0; g < UG; ++g) {
        for (int i = 0; i < 16; ++i) {
            const int u = 16 * g + i;
            float av = 0.0f, dv = 0.0f;
            if (u < H1) {
                float a = 0.0f;
#pragma unroll
                for (int k = 0; k < NIN; ++k) a = fmaf(xi[k], w1t[u][k], a);
                const float pre = a + b1[u];
                const float kf = (float)(unsigned)((u < 64 ? keep_lo >> u : keep_hi >> (u - 64)) & 1ull);
                av = fmaxf(pre, 0.0f) / kp * kf;
                float dd = 0.0f;
#pragma unroll
                for (int j = 0; j < H2; ++j) dd = fmaf(g2[j], W2[u * H2 + j], dd);
                dv = pre > 0.0f ? dd * kf / kp : 0.0f;
            } else if (u == H1) {
                av = valid ? 1.0f : 0.0f;            // the row of ones: row 100 of the product is db_2
            }
            a1c[lane][i] = av;
            dp1c[lane][i] = dv;
        }
        __syncthreads();
        floatx4 acc1 = floatx4{0.0f, 0.0f, 0.0f, 0.0f}, acc2a = acc1, acc2b = acc1;
#pragma unroll 4
        for (int kk = 0; kk < ROWS / 4; ++kk) {
            const int rk = 4 * kk + quad;
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[rk][col], dp1c[rk][col], acc1, 0, 0, 0);
            const float a = a1c[rk][col];
            acc2a = __builtin_amdgcn_mfma_f32_16x16x4f32(a, dp2s[rk][col], acc2a, 0, 0, 0);
            acc2b = __builtin_amdgcn_mfma_f32_16x16x4f32(a, dp2s[rk][16 + col], acc2b, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = 4 * quad + q, u = 16 * g + col;            // dW_1: row f of [X | 1], unit u
            if (u < H1) {
                if (f < NIN) bp[f * H1 + u] = acc1[q];
                else if (f == NIN) bp[OFF_B1 + u] = acc1[q];
            }
            const int unit = 16 * g + 4 * quad + q;                  // dW_2: row unit of [d_1 | 1], columns col and 16 + col
            if (unit < H1) {
                bp[OFF_W2 + unit * H2 + col] = acc2a[q];
                if (col < H2 - 16) bp[OFF_W2 + unit * H2 + 16 + col] = acc2b[q];
            } else if (unit == H1) {
                bp[OFF_B2 + col] = acc2a[q];
                if (col < H2 - 16) bp[OFF_B2 + 16 + col] = acc2b[q];
            }
        }
        __syncthreads();
    }
}

// thread i < 3541: element i of the gradient; thread 3541: the loss.  Block order, one writer each.
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ part, const float* __restrict__ lossp, const int nblocks, const long long n,
                                                     float* __restrict__ grad, float* __restrict__ loss) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < NW) {
        float s = part[i];
#pragma unroll 8
        for (int b = 1; b < nblocks; ++b) s += part[(size_t)b * NW + i];     // the loads are independent; the additions keep block order
        grad[i] = s;
    } else if (i == NW) {
        float s = lossp[0];
        for (int b = 1; b < nblocks; ++b) s += lossp[b];
        *loss = s / (float)n;
    }
}

__global__ __launch_bounds__(256) void mask_kernel(unsigned char* __restrict__ out, const long long n, const float kp, const uint64_t key) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * MASKW) return;
    const long long row = i / MASKW;
    const int unit = int(i - row * MASKW);
    out[i] = (unsigned char)keep_from(pair_hash(key, row, unit >> 1), unit & 1, kp);
}

}  // namespace dmct

struct dm_cluster_trainer {
    static constexpr int SLOTS = 4;                                  // pinned id buffers of the steps in flight
    int device = 0;
    int64_t max_batch = 0;
    hipStream_t stream = nullptr;
    float *d_w = nullptr, *d_m = nullptr, *d_v = nullptr, *d_grad = nullptr, *d_part = nullptr, *d_lossp = nullptr;
    float *d_x = nullptr, *d_y = nullptr, *d_out = nullptr, *d_loss = nullptr;
    unsigned char* d_mask = nullptr;                                 // [max_batch][120]: an explicit mask, or dm_cluster_trainer_mask's result
    long long* d_ids = nullptr;
    long long* h_ids[SLOTS] = {};
    hipEvent_t ev[SLOTS] = {};
    bool ev_used[SLOTS] = {};
    float *d_X = nullptr, *d_Y = nullptr;                            // dm_cluster_trainer_set_data
    int64_t n_data = -1;
    float* d_losses = nullptr;                                       // the loss of step t_base + i
    int64_t losses_cap = 0, t_base = 0, t = 0;
};

namespace {

int ctrainer_check_finite(const char* what, const float* a, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(a[i])) return fail(DM_EINVAL, "dm_cluster_trainer: NaN or Inf in %s (element %zu); nothing was computed", what, i);
    return DM_OK;
}

int ctrainer_check_kp(float kp) {
    if (!(kp > 0.0f && kp <= 1.0f)) return fail(DM_EINVAL, "dm_cluster_trainer: keep_prob %g outside (0, 1]", double(kp));
    return DM_OK;
}

int ctrainer_check_n(dm_cluster_trainer* tr, int64_t n) {
    if (n < 0) return fail(DM_EINVAL, "negative row count");
    if (n > tr->max_batch) return fail(DM_EINVAL, "dm_cluster_trainer: %lld rows exceed max_batch = %lld", (long long)n, (long long)tr->max_batch);
    return DM_OK;
}

// forward + backward + reduction of n rows: leaves out, the gradient and *d_loss_out on the device
void ctrainer_launch_grad(dm_cluster_trainer* tr, const float* dx, const float* dy, const long long* dids, int64_t n_src, int64_t n, float kp,
                          const unsigned char* dmask, uint64_t key, float* d_loss_out) {
    using namespace dmct;
    const int blocks = int((n + ROWS - 1) / ROWS);
    hipLaunchKernelGGL(grad_kernel, dim3(blocks), dim3(ROWS), 0, tr->stream, tr->d_w, dx, dy, dids, (long long)n_src, (long long)n, kp, dmask, key,
                       tr->d_out, tr->d_part, tr->d_lossp);
    hipLaunchKernelGGL(reduce_kernel, dim3((NW + 1 + 255) / 256), dim3(256), 0, tr->stream, tr->d_part, tr->d_lossp, blocks, (long long)n, tr->d_grad,
                       d_loss_out);
}

int ctrainer_launch_adam(dm_cluster_trainer* tr) {
    const int64_t t = tr->t + 1;
    const double lr = 1e-3 * std::sqrt(1.0 - std::pow(0.999, double(t))) / (1.0 - std::pow(0.9, double(t)));
    hipLaunchKernelGGL(dmtrain::adam_kernel, dim3((dmct::NW + 255) / 256), dim3(256), 0, tr->stream, tr->d_w, tr->d_m, tr->d_v, tr->d_grad, float(lr),
                       dmct::NW);
    HIP_TRY(hipGetLastError());
    tr->t = t;
    return DM_OK;
}

int ctrainer_fit_losses(dm_cluster_trainer* tr, int64_t count) {
    if (count <= tr->losses_cap) return DM_OK;
    const int64_t cap = std::max<int64_t>(1024, 2 * count);
    float* nl = nullptr;
    HIP_TRY(hipMalloc(&nl, size_t(cap) * sizeof(float)));
    if (tr->d_losses && tr->losses_cap) {
        hipError_t e = hipMemcpyAsync(nl, tr->d_losses, size_t(tr->losses_cap) * sizeof(float), hipMemcpyDeviceToDevice, tr->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(tr->stream);
        if (e != hipSuccess) {
            (void)hipFree(nl);
            return fail(DM_EDEVICE, "dm_cluster_trainer: growing the loss record failed: %s", hipGetErrorString(e));
        }
    }
    (void)hipFree(tr->d_losses);
    tr->d_losses = nl;
    tr->losses_cap = cap;
    return DM_OK;
}

int ctrainer_init(dm_cluster_trainer* tr, const float* weights) {
    using namespace dmct;
    HIP_TRY(hipSetDevice(tr->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, tr->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DM_EDEVICE, "device %d is %s; this library is built for gfx950 only", tr->device, prop.gcnArchName);
    HIP_TRY(hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking));
    const size_t cap = size_t(tr->max_batch), f = sizeof(float), blocks = (cap + ROWS - 1) / ROWS;
    HIP_TRY(hipMalloc(&tr->d_w, NW * f));
    HIP_TRY(hipMalloc(&tr->d_m, NW * f));
    HIP_TRY(hipMalloc(&tr->d_v, NW * f));
    HIP_TRY(hipMalloc(&tr->d_grad, NW * f));
    HIP_TRY(hipMalloc(&tr->d_part, blocks * NW * f));
    HIP_TRY(hipMalloc(&tr->d_lossp, blocks * f));
    HIP_TRY(hipMalloc(&tr->d_x, cap * NIN * f));
    HIP_TRY(hipMalloc(&tr->d_y, cap * f));
    HIP_TRY(hipMalloc(&tr->d_out, cap * f));
    HIP_TRY(hipMalloc(&tr->d_loss, f));
    HIP_TRY(hipMalloc(&tr->d_mask, cap * MASKW));
    HIP_TRY(hipMalloc(&tr->d_ids, cap * sizeof(long long)));
    for (int i = 0; i < dm_cluster_trainer::SLOTS; ++i) {
        HIP_TRY(hipHostMalloc(&tr->h_ids[i], cap * sizeof(long long)));
        HIP_TRY(hipEventCreateWithFlags(&tr->ev[i], hipEventDisableTiming));
    }
    HIP_TRY(hipMemcpy(tr->d_w, weights, NW * f, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(tr->d_m, 0, NW * f));
    HIP_TRY(hipMemset(tr->d_v, 0, NW * f));
    HIP_TRY(hipMemset(tr->d_grad, 0, NW * f));
    return DM_OK;
}

}  // namespace

extern "C" {

dm_cluster_trainer* dm_cluster_trainer_create(int device, const float* weights, size_t n_floats, int64_t max_batch) {
    if (!weights || n_floats != DM_CLUSTER_WEIGHT_FLOATS) {
        fail(DM_EINVAL, "cluster weights: expected %d floats, got %zu", DM_CLUSTER_WEIGHT_FLOATS, n_floats);
        return nullptr;
    }
    if (max_batch < 1 || max_batch > dmct::MAX_BATCH) {
        fail(DM_EINVAL, "dm_cluster_trainer_create: max_batch %lld outside [1, 2^16]", (long long)max_batch);
        return nullptr;
    }
    if (ctrainer_check_finite("the weights", weights, n_floats) != DM_OK) return nullptr;
    dm_cluster_trainer* tr = new (std::nothrow) dm_cluster_trainer();
    if (!tr) {
        fail(DM_ENOMEM, "out of host memory");
        return nullptr;
    }
    tr->device = device;
    tr->max_batch = max_batch;
    if (ctrainer_init(tr, weights) != DM_OK) {
        std::string keep = g_err;
        dm_cluster_trainer_destroy(tr);
        g_err = keep;
        return nullptr;
    }
    return tr;
}

void dm_cluster_trainer_destroy(dm_cluster_trainer* tr) {
    if (!tr) return;
    (void)hipSetDevice(tr->device);
    if (tr->stream) (void)hipStreamSynchronize(tr->stream);
    float* bufs[] = {tr->d_w, tr->d_m, tr->d_v, tr->d_grad, tr->d_part, tr->d_lossp, tr->d_x, tr->d_y, tr->d_out, tr->d_loss, tr->d_X, tr->d_Y, tr->d_losses};
    for (float* p : bufs) (void)hipFree(p);
    (void)hipFree(tr->d_mask);
    (void)hipFree(tr->d_ids);
    for (int i = 0; i < dm_cluster_trainer::SLOTS; ++i) {
        if (tr->h_ids[i]) (void)hipHostFree(tr->h_ids[i]);
        if (tr->ev[i]) (void)hipEventDestroy(tr->ev[i]);
    }
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    delete tr;
}

int dm_cluster_trainer_set_data(dm_cluster_trainer* tr, const float* x, const float* y, int64_t n_rows) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    if (n_rows < 1 || !x || !y) return fail(DM_EINVAL, "dm_cluster_trainer_set_data: no rows");
    int rc = ctrainer_check_finite("x", x, size_t(n_rows) * dmct::NIN);
    if (rc == DM_OK) rc = ctrainer_check_finite("y", y, size_t(n_rows));
    if (rc) return rc;
    HIP_TRY(hipSetDevice(tr->device));
    HIP_TRY(hipStreamSynchronize(tr->stream));
    float *nx = nullptr, *ny = nullptr;
    HIP_TRY(hipMalloc(&nx, size_t(n_rows) * dmct::NIN * sizeof(float)));
    hipError_t e = hipMalloc(&ny, size_t(n_rows) * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(nx, x, size_t(n_rows) * dmct::NIN * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ny, y, size_t(n_rows) * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(nx);
        (void)hipFree(ny);
        return fail(DM_EDEVICE, "dm_cluster_trainer_set_data: %s", hipGetErrorString(e));
    }
    (void)hipFree(tr->d_X);
    (void)hipFree(tr->d_Y);
    tr->d_X = nx;
    tr->d_Y = ny;
    tr->n_data = n_rows;
    return DM_OK;
}

int dm_cluster_trainer_grad(dm_cluster_trainer* tr, const float* x, const float* y, int64_t n, float keep_prob, const uint8_t* keep, uint64_t seed,
                            int64_t step, float* loss, float* out, float* grad) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    int rc = ctrainer_check_n(tr, n);
    if (rc) return rc;
    if (n == 0) return DM_OK;
    if (!x || !y) return fail(DM_EINVAL, "dm_cluster_trainer_grad: null x or y");
    if ((rc = ctrainer_check_kp(keep_prob)) != DM_OK) return rc;
    if (step < 0) return fail(DM_EINVAL, "dm_cluster_trainer_grad: negative step");
    if ((rc = ctrainer_check_finite("x", x, size_t(n) * dmct::NIN)) != DM_OK) return rc;
    if ((rc = ctrainer_check_finite("y", y, size_t(n))) != DM_OK) return rc;
    if (keep)
        for (size_t i = 0; i < size_t(n) * dmct::MASKW; ++i)
            if (keep[i] > 1) return fail(DM_EINVAL, "dm_cluster_trainer_grad: keep[%zu] = %d is neither 0 nor 1", i, int(keep[i]));
    HIP_TRY(hipSetDevice(tr->device));
    hipStream_t s = tr->stream;
    HIP_TRY(hipMemcpyAsync(tr->d_x, x, size_t(n) * dmct::NIN * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tr->d_y, y, size_t(n) * sizeof(float), hipMemcpyHostToDevice, s));
    if (keep) HIP_TRY(hipMemcpyAsync(tr->d_mask, keep, size_t(n) * dmct::MASKW, hipMemcpyHostToDevice, s));
    ctrainer_launch_grad(tr, tr->d_x, tr->d_y, nullptr, n, n, keep_prob, keep ? tr->d_mask : nullptr, dmct::mask_key(seed, uint64_t(step)), tr->d_loss);
    HIP_TRY(hipGetLastError());
    float l = 0.0f;
    HIP_TRY(hipMemcpyAsync(&l, tr->d_loss, sizeof(float), hipMemcpyDeviceToHost, s));
    if (out) HIP_TRY(hipMemcpyAsync(out, tr->d_out, size_t(n) * sizeof(float), hipMemcpyDeviceToHost, s));
    if (grad) HIP_TRY(hipMemcpyAsync(grad, tr->d_grad, dmct::NW * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (loss) *loss = l;
    if (!std::isfinite(l)) return fail(DM_EINVAL, "dm_cluster_trainer_grad: the loss of this batch is not finite (%g); the state is unchanged", double(l));
    return DM_OK;
}

int dm_cluster_trainer_adam(dm_cluster_trainer* tr, const float* grad) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    if (!grad) return fail(DM_EINVAL, "dm_cluster_trainer_adam: null gradient");
    HIP_TRY(hipSetDevice(tr->device));
    HIP_TRY(hipMemcpyAsync(tr->d_grad, grad, dmct::NW * sizeof(float), hipMemcpyHostToDevice, tr->stream));
    const int rc = ctrainer_launch_adam(tr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(tr->stream));
    tr->t_base = tr->t;                              // a step without a loss: the record starts again behind it
    return DM_OK;
}

int dm_cluster_trainer_step(dm_cluster_trainer* tr, const int64_t* ids, int64_t n, float keep_prob, uint64_t seed) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    if (tr->n_data < 1) return fail(DM_EINVAL, "dm_cluster_trainer_step: no data (dm_cluster_trainer_set_data comes first)");
    int rc = ctrainer_check_n(tr, n);
    if (rc) return rc;
    if (n == 0) return DM_OK;
    if (!ids) return fail(DM_EINVAL, "dm_cluster_trainer_step: null ids");
    if ((rc = ctrainer_check_kp(keep_prob)) != DM_OK) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= tr->n_data)
            return fail(DM_EINVAL, "dm_cluster_trainer_step: ids[%lld] = %lld outside [0, %lld); the state is unchanged", (long long)i, (long long)ids[i],
                        (long long)tr->n_data);
    HIP_TRY(hipSetDevice(tr->device));
    const int64_t rec = tr->t - tr->t_base;
    if ((rc = ctrainer_fit_losses(tr, rec + 1)) != DM_OK) return rc;
    const int slot = int(tr->t % dm_cluster_trainer::SLOTS);
    if (tr->ev_used[slot]) HIP_TRY(hipEventSynchronize(tr->ev[slot]));        // the copy of four steps ago: long done
    std::memcpy(tr->h_ids[slot], ids, size_t(n) * sizeof(long long));
    HIP_TRY(hipMemcpyAsync(tr->d_ids, tr->h_ids[slot], size_t(n) * sizeof(long long), hipMemcpyHostToDevice, tr->stream));
    HIP_TRY(hipEventRecord(tr->ev[slot], tr->stream));
    tr->ev_used[slot] = true;
    ctrainer_launch_grad(tr, tr->d_X, tr->d_Y, tr->d_ids, tr->n_data, n, keep_prob, nullptr, dmct::mask_key(seed, uint64_t(tr->t)), tr->d_losses + rec);
    HIP_TRY(hipGetLastError());
    return ctrainer_launch_adam(tr);
}

int dm_cluster_trainer_losses(dm_cluster_trainer* tr, int64_t first_step, int64_t count, float* losses) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    if (count < 0) return fail(DM_EINVAL, "negative count");
    if (count == 0) return DM_OK;
    if (!losses) return fail(DM_EINVAL, "dm_cluster_trainer_losses: null buffer");
    if (first_step < tr->t_base || first_step + count > tr->t)
        return fail(DM_EINVAL, "dm_cluster_trainer_losses: steps [%lld, %lld) are not all among the recorded steps [%lld, %lld)", (long long)first_step,
                    (long long)(first_step + count), (long long)tr->t_base, (long long)tr->t);
    HIP_TRY(hipSetDevice(tr->device));
    HIP_TRY(hipMemcpyAsync(losses, tr->d_losses + (first_step - tr->t_base), size_t(count) * sizeof(float), hipMemcpyDeviceToHost, tr->stream));
    HIP_TRY(hipStreamSynchronize(tr->stream));
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(losses[i]))
            return fail(DM_EINVAL, "dm_cluster_trainer_losses: the loss of step %lld is not finite (%g); that step and every later one have been applied",
                        (long long)(first_step + i), double(losses[i]));
    return DM_OK;
}

int dm_cluster_trainer_mask(dm_cluster_trainer* tr, uint64_t seed, int64_t step, int64_t n, float keep_prob, uint8_t* keep) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    int rc = ctrainer_check_n(tr, n);
    if (rc) return rc;
    if (n == 0) return DM_OK;
    if (!keep) return fail(DM_EINVAL, "dm_cluster_trainer_mask: null buffer");
    if ((rc = ctrainer_check_kp(keep_prob)) != DM_OK) return rc;
    if (step < 0) return fail(DM_EINVAL, "dm_cluster_trainer_mask: negative step");
    HIP_TRY(hipSetDevice(tr->device));
    const long long total = (long long)n * dmct::MASKW;
    hipLaunchKernelGGL(dmct::mask_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, tr->stream, tr->d_mask, (long long)n, keep_prob,
                       dmct::mask_key(seed, uint64_t(step)));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(keep, tr->d_mask, size_t(total), hipMemcpyDeviceToHost, tr->stream));
    HIP_TRY(hipStreamSynchronize(tr->stream));
    return DM_OK;
}

int dm_cluster_trainer_get_state(dm_cluster_trainer* tr, float* weights, float* m, float* v, int64_t* t) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    HIP_TRY(hipSetDevice(tr->device));
    const size_t bytes = dmct::NW * sizeof(float);
    if (weights) HIP_TRY(hipMemcpyAsync(weights, tr->d_w, bytes, hipMemcpyDeviceToHost, tr->stream));
    if (m) HIP_TRY(hipMemcpyAsync(m, tr->d_m, bytes, hipMemcpyDeviceToHost, tr->stream));
    if (v) HIP_TRY(hipMemcpyAsync(v, tr->d_v, bytes, hipMemcpyDeviceToHost, tr->stream));
    HIP_TRY(hipStreamSynchronize(tr->stream));
    if (t) *t = tr->t;
    return DM_OK;
}

int dm_cluster_trainer_set_state(dm_cluster_trainer* tr, const float* weights, const float* m, const float* v, int64_t t) {
    if (!tr) return fail(DM_EINVAL, "null cluster trainer");
    if (t < 0) return fail(DM_EINVAL, "dm_cluster_trainer_set_state: negative step count");
    HIP_TRY(hipSetDevice(tr->device));
    const size_t bytes = dmct::NW * sizeof(float);
    if (weights) HIP_TRY(hipMemcpyAsync(tr->d_w, weights, bytes, hipMemcpyHostToDevice, tr->stream));
    if (m) HIP_TRY(hipMemcpyAsync(tr->d_m, m, bytes, hipMemcpyHostToDevice, tr->stream));
    if (v) HIP_TRY(hipMemcpyAsync(tr->d_v, v, bytes, hipMemcpyHostToDevice, tr->stream));
    HIP_TRY(hipStreamSynchronize(tr->stream));
    tr->t = tr->t_base = t;
    return DM_OK;
}

}  // extern "C"
