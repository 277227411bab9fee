// xygather.hip.inc — train --resident, device part (part of offline.hip): the windows of a resident set by id.
//
// The training files of a run are segments of one dm_xyset (xyparse.hip.inc).  A window's ID is its index over the concatenated segments:
// segment s holds the ids [win_off[s], win_off[s + 1]) in the order of its centres, so id -> s is a search over the window prefix sums and
// id itself indexes the set's centre block (centres are relative to their segment's first row, row_off[s]).
//   xg_gather_kernel   a block takes WPB consecutive windows of the batch: its first WPB lanes resolve one id each (binary search over
//                      off[0 .. S], 64-bit throughout) to the float offset of the window's first row, (row_off[s] + centre[id] - 10) * 7, in
//                      LDS; then all lanes copy the block's WPB * 147 floats, flat index -> consecutive lanes write consecutive dwords of x and
//                      read consecutive dwords of a window's 588 contiguous source bytes.  A window starts at a multiple of 28 bytes in the
//                      source and of 588 in x, so neither side is 16-byte aligned in general: the copy stays one dword per lane.
//                      An id outside [0, off[S]) writes zeros for its window and raises *bad to n - (its position) by an integer atomicMax,
//                      so that the smallest offending position comes back (0: none).  No float atomics; one writer per element of x.
// dm_xyset_gather runs it on the set's stream into host or device x.  dm_trainer_step_set / dm_trainer_grad_set run it on the trainer's stream
// into the trainer's d_x, *bad being the word behind the finite check's flag: trainer_grad_staged reads both back in the one copy it makes
// anyway, and from there on the step is dm_trainer_step's own code.
#pragma once
#include "host.h"
#include "train.hip.inc"
#include "xyparse.hip.inc"

namespace xgk {

constexpr int THREADS = 256;
constexpr int WPB = 16;                                 // windows per block
constexpr int WFLOATS = DM_WINDOW * DM_NFEAT;           // 147
constexpr int64_t MAX_GATHER = int64_t(1) << 32;        // windows of one dm_xyset_gather (the grid's x is 32-bit)

__global__ __launch_bounds__(THREADS) void xg_gather_kernel(const float* __restrict__ feats, const int* __restrict__ centre, const long long* __restrict__ off,
                                                           const int n_seg, const long long* __restrict__ ids, const long long n, float* __restrict__ x,
                                                           unsigned long long* __restrict__ bad) {
    __shared__ long long base[WPB];
    const long long w0 = (long long)blockIdx.x * WPB;
    if (threadIdx.x < WPB) {
        const long long w = w0 + threadIdx.x;
        long long b = -1;
        if (w < n) {
            const long long id = ids[w];
            if (id >= 0 && id < off[n_seg]) {
                int lo = 0, hi = n_seg;                 // off[lo] <= id < off[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (off[mid] <= id) lo = mid;
                    else hi = mid;
                }
                b = (off[n_seg + 1 + lo] + (long long)centre[id] - xlk::HALF) * DM_NFEAT;
            } else {
                atomicMax(bad, (unsigned long long)(n - w));
            }
        }
        base[threadIdx.x] = b;
    }
    __syncthreads();
    const long long left = n - w0;
    const int span = int(left < WPB ? left : WPB) * WFLOATS;
    float* __restrict__ dst = x + w0 * WFLOATS;
    for (int i = threadIdx.x; i < span; i += THREADS) {
        const int k = i / WFLOATS;
        const long long b = base[k];
        dst[i] = b >= 0 ? feats[b + (i - k * WFLOATS)] : 0.0f;
    }
}

// the segments' prefix sums on the device: off[0 .. S] windows, off[S + 1 .. 2 S + 1] rows; uploaded again when segments were appended since
int set_offsets(dm_xyset* s) {
    const int64_t S = int64_t(s->win_off.size()) - 1;
    if (s->d_off && s->d_off_segs == S) return DM_OK;
    const size_t words = size_t(2 * (S + 1));
    if (words > s->cap_off) {
        if (s->d_off) (void)hipFree(s->d_off);
        s->d_off = nullptr;
        s->cap_off = 0;
        s->d_off_segs = -1;
        const size_t want = 2 * words + 32;
        if (hipMalloc(&s->d_off, want * 8) != hipSuccess) {
            (void)hipGetLastError();
            return fail(DM_ENOMEM, "dm_xyset: hipMalloc(%zu) for the segment table failed", want * 8);
        }
        s->cap_off = want;
    }
    s->off_host.assign(s->win_off.begin(), s->win_off.end());
    s->off_host.insert(s->off_host.end(), s->row_off.begin(), s->row_off.end());
    HIP_TRY(hipMemcpyAsync(s->d_off, s->off_host.data(), words * 8, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));           // the next reader may be on another stream (the trainer's)
    s->d_off_segs = S;
    return DM_OK;
}

void launch_gather(dm_xyset* s, const long long* d_ids, int64_t n, float* d_x, unsigned long long* d_bad, hipStream_t stream) {
    hipLaunchKernelGGL(xg_gather_kernel, dim3(unsigned((n + WPB - 1) / WPB)), dim3(THREADS), 0, stream, s->feats, s->centre, s->d_off, int(s->d_off_segs),
                       d_ids, (long long)n, d_x, d_bad);
}

// the one line for an id outside the set; word = n - position as the kernel raised it
int bad_id(const char* who, dm_xyset* s, const int64_t* ids, int64_t n, long long word) {
    const int64_t at = n - word;
    long long id = 0;
    if (is_device_ptr(ids)) {
        if (hipMemcpy(&id, ids + at, 8, hipMemcpyDeviceToHost) != hipSuccess) (void)hipGetLastError();
    } else {
        id = ids[at];
    }
    return fail(DM_EINVAL, "%s: id %lld at position %lld is outside the %lld windows of the set; nothing was computed", who, id, (long long)at,
                (long long)s->win_off.back());
}

// ids and y to the trainer's blocks, the windows into d_x: what trainer_upload stages for a host-fed step
int trainer_stage_set(dm_trainer* tr, dm_xyset* s, const int64_t* ids, const float* y, int64_t n) {
    if (!ids || !y) return fail(DM_EINVAL, "dm_trainer: null ids or y");
    if (s->device != tr->device) return fail(DM_EINVAL, "dm_trainer: the set is on device %d, the trainer on device %d", s->device, tr->device);
    if (n > tr->max_batch) return fail(DM_EINVAL, "dm_trainer: %lld windows exceed max_batch = %lld", (long long)n, (long long)tr->max_batch);
    HIP_TRY(hipSetDevice(tr->device));
    int rc = set_offsets(s);
    if (rc) return rc;
    hipStream_t st = tr->stream;
    HIP_TRY(hipMemcpyAsync(tr->d_ids, ids, size_t(n) * 8, is_device_ptr(ids) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    rc = trainer_upload(tr, tr->d_y, y, size_t(n) * 2);
    if (rc) return rc;
    unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(tr->d_flag) + 8);
    HIP_TRY(hipMemsetAsync(d_bad, 0, 8, st));
    launch_gather(s, tr->d_ids, n, tr->d_x, d_bad, st);
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

int trainer_grad_set(dm_trainer* tr, dm_xyset* s, const int64_t* ids, const float* y, int64_t n, int unbalanced, float* loss) {
    int rc = trainer_stage_set(tr, s, ids, y, n);
    if (rc) return rc;
    long long word = 0;
    rc = trainer_grad_staged(tr, n, unbalanced, loss, &word);
    if (rc == DM_EINVAL && word != 0) return bad_id("dm_trainer", s, ids, n, word);
    return rc;
}

}  // namespace xgk

extern "C" {

int dm_xyset_gather(dm_xyset* s, const int64_t* ids, int64_t n, float* x) {
    if (!s) return fail(DM_EINVAL, "null handle");
    if (n < 0 || n > xgk::MAX_GATHER) return fail(DM_EINVAL, "dm_xyset_gather: %lld windows", (long long)n);
    if (n == 0) return DM_OK;
    if (!ids || !x) return fail(DM_EINVAL, "dm_xyset_gather: null ids or x");
    HIP_TRY(hipSetDevice(s->device));
    int rc = xgk::set_offsets(s);
    if (rc) return rc;
    const bool id_dev = is_device_ptr(ids), x_dev = is_device_ptr(x);
    const size_t floats = size_t(n) * xgk::WFLOATS;
    if (!s->g_bad && hipMalloc(&s->g_bad, 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DM_ENOMEM, "dm_xyset_gather: hipMalloc(8) failed");
    }
    if (!id_dev && (rc = s->gather.ensure(dm_xyset::G_IDS, size_t(n) * 8)) != DM_OK) return rc;
    if (!x_dev && (rc = s->gather.ensure(dm_xyset::G_X, floats * 4)) != DM_OK) return rc;
    const long long* d_ids = reinterpret_cast<const long long*>(ids);
    if (!id_dev) {
        HIP_TRY(hipMemcpyAsync(s->gather.buf[dm_xyset::G_IDS], ids, size_t(n) * 8, hipMemcpyHostToDevice, s->stream));
        d_ids = s->gather.ptr<const long long>(dm_xyset::G_IDS);
    }
    float* d_x = x_dev ? x : s->gather.ptr<float>(dm_xyset::G_X);
    HIP_TRY(hipMemsetAsync(s->g_bad, 0, 8, s->stream));
    xgk::launch_gather(s, d_ids, n, d_x, static_cast<unsigned long long*>(s->g_bad), s->stream);
    HIP_TRY(hipGetLastError());
    long long word = 0;
    HIP_TRY(hipMemcpyAsync(&word, s->g_bad, 8, hipMemcpyDeviceToHost, s->stream));
    if (!x_dev) HIP_TRY(hipMemcpyAsync(x, d_x, floats * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (word != 0) return xgk::bad_id("dm_xyset_gather", s, ids, n, word);
    return DM_OK;
}

int dm_trainer_grad_set(dm_trainer* tr, dm_xyset* s, const int64_t* ids, const float* y, int64_t n, int unbalanced, float* loss, float* prob, float* grad) {
    if (!tr || !s) return fail(DM_EINVAL, "null handle");
    if (n < 0) return fail(DM_EINVAL, "negative window count");
    if (n == 0) return DM_OK;
    int rc = xgk::trainer_grad_set(tr, s, ids, y, n, unbalanced, loss);
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

int dm_trainer_step_set(dm_trainer* tr, dm_xyset* s, const int64_t* ids, const float* y, int64_t n, int unbalanced, float* loss) {
    if (!tr || !s) return fail(DM_EINVAL, "null handle");
    if (n < 0) return fail(DM_EINVAL, "negative window count");
    if (n == 0) return DM_OK;
    int rc = trainer_step_begin(tr);
    if (rc) return rc;
    rc = xgk::trainer_grad_set(tr, s, ids, y, n, unbalanced, loss);
    if (rc) return rc;
    return trainer_step_finish(tr);
}

}  // extern "C"
