// train.hip.inc — BiLSTM training for gfx950 (part of offline.hip): forward with a tape, backpropagation through time, Adam.
//
// The network is the reference's training graph (bin/DeepMod_scripts/myMultiBiRNN.py:21-91): two independent stacks of three
// BasicLSTMCell(100, forget_bias = 1), gates i, j, f, o; the forward stack over rows 0..10 of a 21 x 7 window, the backward stack over rows
// 20..10; logits = concat(h_fw[10], h_bw[10]) W[200,2] + b; loss = mean softmax cross entropy (of logits * [0.1, 0.9] when unbalanced).  Only
// the 11 live steps per direction carry gradient - the pruning of the inference kernels.
//
// One precision (fp32), plain GEMM-shaped kernels on v_mfma_f32_16x16x4_f32, plain launches on the trainer's stream, no fusion across
// (layer, step), no float atomics: every output element has one writer and every reduction a fixed order, so two runs are bit-identical.
// All kernels read the weights in the canonical layout of flatten_weights (the blob Adam updates in place), no repack:
//
//   fwd_step_kernel   [n,K] x [K,400] + b per (direction, layer, step), K = 107 | 200; the gate columns are visited unit-major (tile
//                     (g, gate) = units 16 g .. 16 g + 15 of one gate) so a lane holds i, j, f, o of one (window, unit) and the cell is the
//                     lane-local epilogue; post-activation gates, c and h go to the tape.  Units are padded 100 -> 112 (zero operands).
//   head_loss_kernel  logits, softmax, per-window loss, dz and d concat(h) = dz W^T, one thread per window
//   cell_bwd_kernel   elementwise: dG (written over the gates of the tape) and dc_prev
//   bwd_dx_kernel     d[inp, h_prev] = dG [n,400] x W^T; the input part is added to the layer below, the h part is the step before
//   dw_kernel         dW = [XH | 1]^T dG per (direction, layer), split over the 11 steps; the row of ones makes db row K of the product
//   dw_reduce_kernel  the 11 partials summed in step order
//   adam_kernel       TF1 AdamOptimizer, elementwise, contraction off (bit-equal to the numpy statement tests/train_oracle.py:adam_numpy_f32)
//
// Tape: 600 floats per (direction, layer, step, window) = 158,400 B per window: 324 MB at n = 2,048.
// Algorithmic work of a step: 3 x 8.924 MFLOP per window (forward, dX, dW).
#pragma once
#include "host.h"

namespace dmtrain {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int HID = 100, NFEAT = 7, WIN = 21, LIVE = 11, NG = 400;
constexpr int NW = DM_WEIGHT_FLOATS;                 // 408,402
constexpr int NW_LSTM = 408000;                      // everything but the head
constexpr int DIR_FLOATS = 204000;
constexpr int HEAD_W = 408000, HEAD_B = 408400;
constexpr int UG = 7;                                // unit groups of 16 (100 -> 112)

__host__ __device__ inline int kin_of(int layer) { return layer == 0 ? NFEAT : HID; }
__host__ __device__ inline int woff(int d, int layer) { return d * DIR_FLOATS + (layer == 0 ? 0 : 43200 + (layer - 1) * 80400); }
__host__ __device__ inline int slot_of(int d, int layer, int t) { return (d * 3 + layer) * LIVE + t; }

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: one (layer, step) of both directions.  grid (ceil(n / 64), 2), 256 threads; a wave owns 16 windows x all gate columns.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int LEN>
__device__ __forceinline__ void fwd_segment(floatx4 (&acc)[UG][4], const float* __restrict__ src, const float* __restrict__ wrows, const int lane) {
    const int col = lane & 15, quad = lane >> 4;
    constexpr int KS = (LEN + 3) / 4;
#pragma unroll 2
    for (int kk = 0; kk < KS; ++kk) {
        const int k = 4 * kk + quad;
        const bool kv = k < LEN;
        const float a = kv ? src[k] : 0.0f;
        const float* wr = wrows + (size_t)(kv ? k : 0) * NG;
#pragma unroll
        for (int g = 0; g < UG; ++g) {
            const int u = 16 * g + col;
            const bool v = kv && u < HID;
#pragma unroll
            for (int gate = 0; gate < 4; ++gate) {
                const float b = v ? wr[gate * HID + u] : 0.0f;
                acc[g][gate] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[g][gate], 0, 0, 0);
            }
        }
    }
}

template <bool L0>
__global__ __launch_bounds__(256) void fwd_step_kernel(const float* __restrict__ wts, const float* __restrict__ x, float* __restrict__ G,
                                                       float* __restrict__ C, float* __restrict__ H, const long long n, const int layer, const int t) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int d = blockIdx.y;
    const long long m0 = ((long long)blockIdx.x * 4 + wave) * 16;
    if (m0 >= n) return;                                   // no barrier in this kernel
    constexpr int KIN = L0 ? NFEAT : HID;
    const float* Wk = wts + woff(d, layer);
    const float* bias = Wk + (size_t)(KIN + HID) * NG;
    const int slot = slot_of(d, layer, t);
    long long wa = m0 + col;                               // the window whose operand row this lane loads (clamped: its results are not stored)
    if (wa > n - 1) wa = n - 1;

    floatx4 acc[UG][4];
#pragma unroll
    for (int g = 0; g < UG; ++g) {
        const int u = 16 * g + col;
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) {
            const float b = u < HID ? bias[gate * HID + u] : 0.0f;
            acc[g][gate] = floatx4{b, b, b, b};
        }
    }
    if constexpr (L0) {
        const int row = d == 0 ? t : WIN - 1 - t;
        fwd_segment<NFEAT>(acc, x + (size_t)wa * (WIN * NFEAT) + row * NFEAT, Wk, lane);
    } else {
        fwd_segment<HID>(acc, H + ((size_t)slot_of(d, layer - 1, t) * n + wa) * HID, Wk, lane);
    }
    if (t > 0) fwd_segment<HID>(acc, H + ((size_t)(slot - 1) * n + wa) * HID, Wk + (size_t)KIN * NG, lane);

#pragma unroll
    for (int g = 0; g < UG; ++g) {
        const int u = 16 * g + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long w = m0 + 4 * quad + r;
            if (w < n && u < HID) {
                const float cp = t > 0 ? C[((size_t)(slot - 1) * n + w) * HID + u] : 0.0f;
                const float gi = sigmoidf_(acc[g][0][r]);
                const float gj = tanhf(acc[g][1][r]);
                const float gf = sigmoidf_(acc[g][2][r] + 1.0f);          // forget_bias = 1
                const float go = sigmoidf_(acc[g][3][r]);
                const float c = cp * gf + gi * gj;
                const float h = tanhf(c) * go;
                float* gp = G + ((size_t)slot * n + w) * NG + u;
                gp[0] = gi;
                gp[HID] = gj;
                gp[2 * HID] = gf;
                gp[3 * HID] = go;
                C[((size_t)slot * n + w) * HID + u] = c;
                H[((size_t)slot * n + w) * HID + u] = h;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// head: logits, prediction, per-window loss, dz, and dh of the two top cells at step 10.  One thread per window.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_loss_kernel(const float* __restrict__ wts, const float* __restrict__ H, const float* __restrict__ y,
                                                        const long long n, const int unbalanced, float* __restrict__ prob, float* __restrict__ lossw,
                                                        float* __restrict__ dz, float* __restrict__ dh_fw, float* __restrict__ dh_bw) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const float* Wo = wts + HEAD_W;
    const float* hf = H + ((size_t)slot_of(0, 2, LIVE - 1) * n + w) * HID;
    const float* hb = H + ((size_t)slot_of(1, 2, LIVE - 1) * n + w) * HID;
    float z0 = 0.0f, z1 = 0.0f;
    for (int k = 0; k < HID; ++k) {
        z0 = fmaf(hf[k], Wo[2 * k], z0);
        z1 = fmaf(hf[k], Wo[2 * k + 1], z1);
    }
    for (int k = 0; k < HID; ++k) {
        z0 = fmaf(hb[k], Wo[2 * (HID + k)], z0);
        z1 = fmaf(hb[k], Wo[2 * (HID + k) + 1], z1);
    }
    z0 += wts[HEAD_B];
    z1 += wts[HEAD_B + 1];
    if (prob) {                                            // prediction = softmax(z), never the weighted logits
        const float m = fmaxf(z0, z1);
        const float e0 = expf(z0 - m), e1 = expf(z1 - m);
        const float s = e0 + e1;
        prob[2 * w] = e0 / s;
        prob[2 * w + 1] = e1 / s;
    }
    const float cw0 = unbalanced ? 0.1f : 1.0f, cw1 = unbalanced ? 0.9f : 1.0f;
    const float q0 = z0 * cw0, q1 = z1 * cw1;
    const float m = fmaxf(q0, q1);
    const float lse = m + logf(expf(q0 - m) + expf(q1 - m));
    const float y0 = y[2 * w], y1 = y[2 * w + 1];
    lossw[w] = -(y0 * (q0 - lse) + y1 * (q1 - lse));
    const float fn = (float)n;
    const float ys = y0 + y1;
    const float d0 = cw0 * ((expf(q0 - lse) * ys - y0) / fn);
    const float d1 = cw1 * ((expf(q1 - lse) * ys - y1) / fn);
    dz[2 * w] = d0;
    dz[2 * w + 1] = d1;
    float* of = dh_fw + (size_t)w * HID;
    float* ob = dh_bw + (size_t)w * HID;
    for (int k = 0; k < HID; ++k) {
        of[k] = d0 * Wo[2 * k] + d1 * Wo[2 * k + 1];
        ob[k] = d0 * Wo[2 * (HID + k)] + d1 * Wo[2 * (HID + k) + 1];
    }
}

// sum of `n` floats in a fixed order: thread i takes i, i + 256, ...; then a tree over the 256 partials.  One block.
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ lossw, const long long n, float* __restrict__ loss) {
    __shared__ float part[256];
    float s = 0.0f;
    for (long long i = threadIdx.x; i < n; i += 256) s += lossw[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = part[0] / (float)n;
}

// head gradients: output o < 400: dW[k][c] = sum_w hcat[w][k] dz[w][c]; o >= 400: db[c].  One wave per output, fixed order.
__global__ __launch_bounds__(64) void head_grad_kernel(const float* __restrict__ H, const float* __restrict__ dz, const long long n, float* __restrict__ grad) {
    const int o = blockIdx.x;
    const int lane = threadIdx.x;
    float s = 0.0f;
    if (o < 2 * 2 * HID) {
        const int k = o >> 1, c = o & 1;
        const float* h = H + (size_t)slot_of(k < HID ? 0 : 1, 2, LIVE - 1) * n * HID + (k < HID ? k : k - HID);
        for (long long w = lane; w < n; w += 64) s = fmaf(h[(size_t)w * HID], dz[2 * w + c], s);
    } else {
        const int c = o - 2 * 2 * HID;
        for (long long w = lane; w < n; w += 64) s += dz[2 * w + c];
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) grad[HEAD_W + o] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cell backward of one (layer, step), both directions: grid (ceil(n * 100 / 256), 2).  The gates of the tape become dG.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cell_bwd_kernel(float* __restrict__ G, const float* __restrict__ C, const float* __restrict__ dh_all,
                                                       float* __restrict__ dc_all, const long long n, const long long cap, const int layer, const int t) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * HID) return;
    const int d = blockIdx.y;
    const long long w = i / HID;
    const int u = int(i - w * HID);
    const int slot = slot_of(d, layer, t);
    const float* dh = dh_all + (size_t)(d * 3 + layer) * cap * HID;
    float* dcb = dc_all + (size_t)(d * 3 + layer) * cap * HID;
    float* gp = G + ((size_t)slot * n + w) * NG + u;
    const float gi = gp[0], gj = gp[HID], gf = gp[2 * HID], go = gp[3 * HID];
    const float c = C[((size_t)slot * n + w) * HID + u];
    const float cp = t > 0 ? C[((size_t)(slot - 1) * n + w) * HID + u] : 0.0f;
    const float tc = tanhf(c);
    const float dhv = dh[i];
    const float dc = dcb[i] + dhv * go * (1.0f - tc * tc);
    gp[0] = dc * gj * (gi * (1.0f - gi));
    gp[HID] = dc * gi * (1.0f - gj * gj);
    gp[2 * HID] = dc * cp * (gf * (1.0f - gf));
    gp[3 * HID] = dhv * tc * (go * (1.0f - go));
    dcb[i] = dc * gf;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// d[inp, h_prev] = dG W^T of one (layer, step), both directions.  grid (ceil(n / 64), 2), 256 threads, a wave owns 16 windows.
// Output columns [c0, c0 + cnt) of the K: c < kin is the layer's input (added to the dh of the layer below, same step), the others its
// h_prev (the dh of this layer for the step before, overwritten).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void bwd_dx_kernel(const float* __restrict__ wts, const float* __restrict__ G, float* __restrict__ dh_all,
                                                     const long long n, const long long cap, const int layer, const int t, const int c0, const int cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int d = blockIdx.y;
    const long long m0 = ((long long)blockIdx.x * 4 + wave) * 16;
    if (m0 >= n) return;
    const int kin = kin_of(layer);
    const float* Wk = wts + woff(d, layer);
    long long wa = m0 + col;
    if (wa > n - 1) wa = n - 1;
    const float* arow = G + ((size_t)slot_of(d, layer, t) * n + wa) * NG;
    floatx4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
    for (int kk = 0; kk < NG / 4; ++kk) {
        const int k = 4 * kk + quad;
        const float a = arow[k];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int oc = 16 * j + col;
            const float b = oc < cnt ? Wk[(size_t)(c0 + oc) * NG + k] : 0.0f;
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j], 0, 0, 0);
        }
    }
    float* dh_own = dh_all + (size_t)(d * 3 + layer) * cap * HID;
    float* dh_below = layer > 0 ? dh_all + (size_t)(d * 3 + layer - 1) * cap * HID : nullptr;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int oc = 16 * j + col;
        const int c = c0 + oc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long w = m0 + 4 * quad + r;
            if (w < n && oc < cnt) {
                if (c < kin) {
                    if (dh_below) dh_below[(size_t)w * HID + c] += acc[j][r];
                } else {
                    dh_own[(size_t)w * HID + (c - kin)] = acc[j][r];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight gradients: part[t][kernel | bias of (d, l)] = [XH_t | 1]^T dG_t.  grid (5 column groups of 80, 13 row tiles, 6 x 11), one wave.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void dw_kernel(const float* __restrict__ x, const float* __restrict__ G, const float* __restrict__ H,
                                                const long long n, float* __restrict__ part) {
    const int lane = threadIdx.x;
    const int col = lane & 15, quad = lane >> 4;
    const int cg = blockIdx.x, mt = blockIdx.y;
    const int dl = blockIdx.z / LIVE, t = blockIdx.z % LIVE;
    const int d = dl / 3, layer = dl % 3;
    const int kin = kin_of(layer), K = kin + HID;
    if (16 * mt > K) return;                               // rows 0 .. K (row K = the bias)
    const int slot = slot_of(d, layer, t);
    // the operand row of this lane: one row of [inp | h_prev | 1] for every window
    const int kidx = 16 * mt + col;
    const float* src = nullptr;
    size_t stride = 0;
    float cval = 0.0f;
    if (kidx < kin) {
        if (layer == 0) {
            src = x + (d == 0 ? t : WIN - 1 - t) * NFEAT + kidx;
            stride = WIN * NFEAT;
        } else {
            src = H + (size_t)slot_of(d, layer - 1, t) * n * HID + kidx;
            stride = HID;
        }
    } else if (kidx < K) {
        if (t > 0) {
            src = H + (size_t)(slot - 1) * n * HID + (kidx - kin);
            stride = HID;
        }
    } else if (kidx == K) {
        cval = 1.0f;
    }
    const float* gb = G + (size_t)slot * n * NG + cg * 80 + col;
    floatx4 acc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) acc[j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    const long long steps = (n + 3) / 4;
    for (long long rr = 0; rr < steps; ++rr) {
        const long long w = 4 * rr + quad;
        const bool v = w < n;
        const float a = v ? (src ? src[(size_t)w * stride] : cval) : 0.0f;
        const float* gr = gb + (size_t)(v ? w : 0) * NG;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const float b = v ? gr[16 * j] : 0.0f;
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[j], 0, 0, 0);
        }
    }
    float* out = part + (size_t)t * NW_LSTM + woff(d, layer);
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * mt + 4 * quad + r;
            if (row <= K) out[(size_t)row * NG + cg * 80 + 16 * j + col] = acc[j][r];
        }
}

__global__ __launch_bounds__(256) void dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NW_LSTM) return;
    float s = part[i];
#pragma unroll
    for (int t = 1; t < LIVE; ++t) s += part[(size_t)t * NW_LSTM + i];
    grad[i] = s;
}

// TF1 AdamOptimizer (training_ops: m, v, then var -= lr_t m / (sqrt(v) + eps)); one rounding per operation, in this order
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                                                   const float lr_t, const int n) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    const float gi = g[i];
    const float mn = b1 * m[i] + omb1 * gi;
    const float vn = b2 * v[i] + omb2 * (gi * gi);
    m[i] = mn;
    v[i] = vn;
    w[i] = w[i] - (lr_t * mn) / (sqrtf(vn) + eps);
}

__global__ __launch_bounds__(256) void finite_check_kernel(const float* __restrict__ a, const long long na, const float* __restrict__ b, const long long nb,
                                                           int* __restrict__ flag) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += (long long)gridDim.x * blockDim.x) {
        const float v = i < na ? a[i] : b[i - na];
        bad |= !(fabsf(v) <= 3.4028234664e38f);            // NaN or Inf
    }
    if (bad) atomicOr(flag, 1);
}

}  // namespace dmtrain

struct dm_trainer {
    int device = 0;
    int64_t max_batch = 0;
    hipStream_t stream = nullptr;
    float *d_w = nullptr, *d_m = nullptr, *d_v = nullptr, *d_grad = nullptr, *d_part = nullptr;
    float *d_G = nullptr, *d_C = nullptr, *d_H = nullptr;           // the tape
    float *d_x = nullptr, *d_y = nullptr, *d_prob = nullptr, *d_lossw = nullptr, *d_dz = nullptr, *d_loss = nullptr;
    float *d_dh = nullptr, *d_dc = nullptr;                       // [2][3][max_batch][100]
    int* d_flag = nullptr;                                        // 16 bytes: the finite check's flag, and at byte 8 the id word of a step from a set
    long long* d_ids = nullptr;                                   // [max_batch]: the window ids of a step from a set (xygather.hip.inc)
    int64_t t = 0;
    // dm_trainer_profile: HIP events around every dm_trainer_step (uploads, the two host round trips for the input check and the loss, Adam)
    bool profile = false, in_step = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double prof_ms = 0.0;
    int64_t prof_steps = 0;
};

namespace {

int trainer_upload(dm_trainer* tr, float* dst, const float* src, size_t floats) {
    HIP_TRY(hipMemcpyAsync(dst, src, floats * sizeof(float), is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, tr->stream));
    return DM_OK;
}
int trainer_download(dm_trainer* tr, float* dst, const float* src, size_t floats) {
    HIP_TRY(hipMemcpyAsync(dst, src, floats * sizeof(float), is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, tr->stream));
    return DM_OK;
}

// d_x and d_y are staged on the stream: finite check, forward, backward: leaves loss, prob and the gradient on the device and *loss on the host.
// Nothing is launched past an error.  bad_id (dm_trainer_step_set, xygather.hip.inc): the word behind the finite flag, which the gather raised
// for an id outside the set, comes back in the same copy.
int trainer_grad_staged(dm_trainer* tr, int64_t n, int unbalanced, float* loss, long long* bad_id = nullptr) {
    using namespace dmtrain;
    hipStream_t s = tr->stream;
    HIP_TRY(hipMemsetAsync(tr->d_flag, 0, sizeof(int), s));
    hipLaunchKernelGGL(finite_check_kernel, dim3(unsigned(std::min<int64_t>((n * WIN * NFEAT + 255) / 256, 1024))), dim3(256), 0, s, tr->d_x,
                       (long long)n * WIN * NFEAT, tr->d_y, (long long)n * 2, tr->d_flag);
    HIP_TRY(hipGetLastError());
    long long back[2] = {0, 0};                                      // the flag in the first int; the id word at byte 8
    HIP_TRY(hipMemcpyAsync(back, tr->d_flag, bad_id ? 16 : sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad_id) {
        *bad_id = back[1];
        if (back[1] != 0) return DM_EINVAL;                          // the caller words it
    }
    int flag = 0;
    std::memcpy(&flag, back, sizeof(int));
    if (flag) return fail(DM_EINVAL, "dm_trainer: NaN or Inf in x or y (%lld windows); nothing was computed", (long long)n);

    const long long nn = n, cap = tr->max_batch;
    const dim3 gw(unsigned((n + 63) / 64), 2), b256(256);
    for (int layer = 0; layer < 3; ++layer)
        for (int t = 0; t < LIVE; ++t) {
            if (layer == 0) hipLaunchKernelGGL(fwd_step_kernel<true>, gw, b256, 0, s, tr->d_w, tr->d_x, tr->d_G, tr->d_C, tr->d_H, nn, layer, t);
            else hipLaunchKernelGGL(fwd_step_kernel<false>, gw, b256, 0, s, tr->d_w, tr->d_x, tr->d_G, tr->d_C, tr->d_H, nn, layer, t);
        }
    HIP_TRY(hipGetLastError());
    // dh of layers 0, 1 and every dc start from zero; dh of the top cells comes from the head
    HIP_TRY(hipMemsetAsync(tr->d_dh, 0, size_t(6) * cap * HID * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(tr->d_dc, 0, size_t(6) * cap * HID * sizeof(float), s));
    hipLaunchKernelGGL(head_loss_kernel, dim3(unsigned((n + 255) / 256)), b256, 0, s, tr->d_w, tr->d_H, tr->d_y, nn, unbalanced ? 1 : 0, tr->d_prob,
                       tr->d_lossw, tr->d_dz, tr->d_dh + size_t(2) * cap * HID, tr->d_dh + size_t(5) * cap * HID);
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), b256, 0, s, tr->d_lossw, nn, tr->d_loss);
    hipLaunchKernelGGL(head_grad_kernel, dim3(402), dim3(64), 0, s, tr->d_H, tr->d_dz, nn, tr->d_grad);
    HIP_TRY(hipGetLastError());
    const dim3 ge(unsigned((n * HID + 255) / 256), 2);
    for (int t = LIVE - 1; t >= 0; --t)
        for (int layer = 2; layer >= 0; --layer) {
            hipLaunchKernelGGL(cell_bwd_kernel, ge, b256, 0, s, tr->d_G, tr->d_C, tr->d_dh, tr->d_dc, nn, cap, layer, t);
            if (layer == 0) {
                if (t > 0) hipLaunchKernelGGL(bwd_dx_kernel<7>, gw, b256, 0, s, tr->d_w, tr->d_G, tr->d_dh, nn, cap, layer, t, NFEAT, HID);
            } else if (t > 0) {
                hipLaunchKernelGGL(bwd_dx_kernel<13>, gw, b256, 0, s, tr->d_w, tr->d_G, tr->d_dh, nn, cap, layer, t, 0, 2 * HID);
            } else {
                hipLaunchKernelGGL(bwd_dx_kernel<7>, gw, b256, 0, s, tr->d_w, tr->d_G, tr->d_dh, nn, cap, layer, t, 0, HID);
            }
        }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dw_kernel, dim3(5, 13, 6 * LIVE), dim3(64), 0, s, tr->d_x, tr->d_G, tr->d_H, nn, tr->d_part);
    hipLaunchKernelGGL(dw_reduce_kernel, dim3((NW_LSTM + 255) / 256), b256, 0, s, tr->d_part, tr->d_grad);
    HIP_TRY(hipGetLastError());
    float l = 0.0f;
    HIP_TRY(hipMemcpyAsync(&l, tr->d_loss, sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (loss) *loss = l;
    if (!std::isfinite(l)) return fail(DM_EINVAL, "dm_trainer: the loss of this batch is not finite (%g); the state is unchanged", double(l));
    return DM_OK;
}

// checks and staging of host or device x and y, then trainer_grad_staged
int trainer_grad_device(dm_trainer* tr, const float* x, const float* y, int64_t n, int unbalanced, float* loss) {
    using namespace dmtrain;
    if (!x || !y) return fail(DM_EINVAL, "dm_trainer: null x or y");
    if (n > tr->max_batch) return fail(DM_EINVAL, "dm_trainer: %lld windows exceed max_batch = %lld", (long long)n, (long long)tr->max_batch);
    HIP_TRY(hipSetDevice(tr->device));
    int rc = trainer_upload(tr, tr->d_x, x, size_t(n) * WIN * NFEAT);
    if (rc) return rc;
    rc = trainer_upload(tr, tr->d_y, y, size_t(n) * 2);
    if (rc) return rc;
    return trainer_grad_staged(tr, n, unbalanced, loss);
}

int trainer_adam_device(dm_trainer* tr) {
    const int64_t t = tr->t + 1;
    const double lr = 1e-3 * std::sqrt(1.0 - std::pow(0.999, double(t))) / (1.0 - std::pow(0.9, double(t)));
    hipLaunchKernelGGL(dmtrain::adam_kernel, dim3((dmtrain::NW + 255) / 256), dim3(256), 0, tr->stream, tr->d_w, tr->d_m, tr->d_v, tr->d_grad, float(lr),
                       dmtrain::NW);
    HIP_TRY(hipGetLastError());
    if (tr->in_step) HIP_TRY(hipEventRecord(tr->ev1, tr->stream));
    HIP_TRY(hipStreamSynchronize(tr->stream));
    tr->t = t;
    return DM_OK;
}

// the two ends of a step (dm_trainer_step, dm_trainer_step_set): the profile's bracket, Adam behind the gradient
int trainer_step_begin(dm_trainer* tr) {
    if (tr->profile) {
        HIP_TRY(hipSetDevice(tr->device));
        HIP_TRY(hipEventRecord(tr->ev0, tr->stream));
    }
    return DM_OK;
}
int trainer_step_finish(dm_trainer* tr) {
    tr->in_step = tr->profile;
    const int rc = trainer_adam_device(tr);
    tr->in_step = false;
    if (rc == DM_OK && tr->profile) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, tr->ev0, tr->ev1));
        tr->prof_ms += ms;
        ++tr->prof_steps;
    }
    return rc;
}

int trainer_init(dm_trainer* tr, const float* weights) {
    using namespace dmtrain;
    HIP_TRY(hipSetDevice(tr->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, tr->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DM_EDEVICE, "device %d is %s; this library is built for gfx950 only", tr->device, prop.gcnArchName);
    HIP_TRY(hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking));
    const size_t cap = size_t(tr->max_batch), f = sizeof(float);
    HIP_TRY(hipMalloc(&tr->d_w, NW * f));
    HIP_TRY(hipMalloc(&tr->d_m, NW * f));
    HIP_TRY(hipMalloc(&tr->d_v, NW * f));
    HIP_TRY(hipMalloc(&tr->d_grad, NW * f));
    HIP_TRY(hipMalloc(&tr->d_part, size_t(LIVE) * NW_LSTM * f));
    HIP_TRY(hipMalloc(&tr->d_G, size_t(6 * LIVE) * cap * NG * f));
    HIP_TRY(hipMalloc(&tr->d_C, size_t(6 * LIVE) * cap * HID * f));
    HIP_TRY(hipMalloc(&tr->d_H, size_t(6 * LIVE) * cap * HID * f));
    HIP_TRY(hipMalloc(&tr->d_x, cap * WIN * NFEAT * f));
    HIP_TRY(hipMalloc(&tr->d_y, cap * 2 * f));
    HIP_TRY(hipMalloc(&tr->d_prob, cap * 2 * f));
    HIP_TRY(hipMalloc(&tr->d_lossw, cap * f));
    HIP_TRY(hipMalloc(&tr->d_dz, cap * 2 * f));
    HIP_TRY(hipMalloc(&tr->d_loss, f));
    HIP_TRY(hipMalloc(&tr->d_dh, size_t(6) * cap * HID * f));
    HIP_TRY(hipMalloc(&tr->d_dc, size_t(6) * cap * HID * f));
    HIP_TRY(hipMalloc(&tr->d_flag, 16));
    HIP_TRY(hipMalloc(&tr->d_ids, cap * sizeof(long long)));
    HIP_TRY(hipMemcpy(tr->d_w, weights, NW * f, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(tr->d_m, 0, NW * f));
    HIP_TRY(hipMemset(tr->d_v, 0, NW * f));
    HIP_TRY(hipMemset(tr->d_grad, 0, NW * f));
    return DM_OK;
}

}  // namespace

extern "C" {

dm_trainer* dm_trainer_create(int device, const float* weights, size_t n_floats, int n_feat, int hidden, int window, int layers, int64_t max_batch) {
    if (!weights || n_floats != DM_WEIGHT_FLOATS) {
        fail(DM_EINVAL, "weights: expected %d floats, got %zu", DM_WEIGHT_FLOATS, n_floats);
        return nullptr;
    }
    if (n_feat != DM_NFEAT || hidden != DM_HIDDEN || window != DM_WINDOW || layers != DM_LAYERS) {
        fail(DM_EINVAL, "unsupported geometry fnum=%d hidden=%d window=%d layers=%d (built for 7/100/21/3)", n_feat, hidden, window, layers);
        return nullptr;
    }
    if (max_batch < 1 || max_batch > (int64_t(1) << 20)) {
        fail(DM_EINVAL, "dm_trainer_create: max_batch %lld outside [1, 2^20]", (long long)max_batch);
        return nullptr;
    }
    dm_trainer* tr = new (std::nothrow) dm_trainer();
    if (!tr) {
        fail(DM_ENOMEM, "out of host memory");
        return nullptr;
    }
    tr->device = device;
    tr->max_batch = max_batch;
    if (trainer_init(tr, weights) != DM_OK) {
        std::string keep = g_err;
        dm_trainer_destroy(tr);
        g_err = keep;
        return nullptr;
    }
    return tr;
}

void dm_trainer_destroy(dm_trainer* tr) {
    if (!tr) return;
    (void)hipSetDevice(tr->device);
    if (tr->stream) (void)hipStreamSynchronize(tr->stream);
    float* bufs[] = {tr->d_w, tr->d_m, tr->d_v, tr->d_grad, tr->d_part, tr->d_G, tr->d_C, tr->d_H, tr->d_x, tr->d_y, tr->d_prob, tr->d_lossw,
                     tr->d_dz, tr->d_loss, tr->d_dh, tr->d_dc};
    for (float* p : bufs) (void)hipFree(p);
    (void)hipFree(tr->d_flag);
    (void)hipFree(tr->d_ids);
    if (tr->ev0) (void)hipEventDestroy(tr->ev0);
    if (tr->ev1) (void)hipEventDestroy(tr->ev1);
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    delete tr;
}

int dm_trainer_grad(dm_trainer* tr, const float* x, const float* y, int64_t n, int unbalanced, float* loss, float* prob, float* grad) {
    if (!tr) return fail(DM_EINVAL, "null trainer");
    if (n < 0) return fail(DM_EINVAL, "negative window count");
    if (n == 0) return DM_OK;
    int rc = trainer_grad_device(tr, x, y, n, unbalanced, loss);
    if (rc) return rc;
    if (prob) {
        rc = trainer_download(tr, prob, tr->d_prob, size_t(n) * 2);
        if (rc) return rc;
    }
    if (grad) {
        rc = trainer_download(tr, grad, tr->d_grad, dmtrain::NW);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(tr->stream));
    return DM_OK;
}

int dm_trainer_adam(dm_trainer* tr, const float* grad) {
    if (!tr) return fail(DM_EINVAL, "null trainer");
    if (!grad) return fail(DM_EINVAL, "dm_trainer_adam: null gradient");
    HIP_TRY(hipSetDevice(tr->device));
    int rc = trainer_upload(tr, tr->d_grad, grad, dmtrain::NW);
    if (rc) return rc;
    return trainer_adam_device(tr);
}

int dm_trainer_step(dm_trainer* tr, const float* x, const float* y, int64_t n, int unbalanced, float* loss) {
    if (!tr) return fail(DM_EINVAL, "null trainer");
    if (n < 0) return fail(DM_EINVAL, "negative window count");
    if (n == 0) return DM_OK;
    int rc = trainer_step_begin(tr);
    if (rc) return rc;
    rc = trainer_grad_device(tr, x, y, n, unbalanced, loss);
    if (rc) return rc;
    return trainer_step_finish(tr);
}

int dm_trainer_profile(dm_trainer* tr, int on, double* step_ms, int64_t* steps) {
    if (!tr) return fail(DM_EINVAL, "null trainer");
    HIP_TRY(hipSetDevice(tr->device));
    if (step_ms) *step_ms = tr->prof_ms;
    if (steps) *steps = tr->prof_steps;
    if (on && !tr->ev0) {
        HIP_TRY(hipEventCreate(&tr->ev0));
        HIP_TRY(hipEventCreate(&tr->ev1));
    }
    tr->profile = on != 0;
    tr->prof_ms = 0.0;
    tr->prof_steps = 0;
    return DM_OK;
}

int dm_trainer_get_state(dm_trainer* tr, float* weights, float* m, float* v, int64_t* t) {
    if (!tr) return fail(DM_EINVAL, "null trainer");
    HIP_TRY(hipSetDevice(tr->device));
    int rc = DM_OK;
    if (weights) rc = trainer_download(tr, weights, tr->d_w, dmtrain::NW);
    if (rc == DM_OK && m) rc = trainer_download(tr, m, tr->d_m, dmtrain::NW);
    if (rc == DM_OK && v) rc = trainer_download(tr, v, tr->d_v, dmtrain::NW);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(tr->stream));
    if (t) *t = tr->t;
    return DM_OK;
}

int dm_trainer_set_state(dm_trainer* tr, const float* weights, const float* m, const float* v, int64_t t) {
    if (!tr) return fail(DM_EINVAL, "null trainer");
    if (t < 0) return fail(DM_EINVAL, "dm_trainer_set_state: negative step count");
    HIP_TRY(hipSetDevice(tr->device));
    int rc = DM_OK;
    if (weights) rc = trainer_upload(tr, tr->d_w, weights, dmtrain::NW);
    if (rc == DM_OK && m) rc = trainer_upload(tr, tr->d_m, m, dmtrain::NW);
    if (rc == DM_OK && v) rc = trainer_upload(tr, tr->d_v, v, dmtrain::NW);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(tr->stream));
    tr->t = t;
    return DM_OK;
}

}  // extern "C"
