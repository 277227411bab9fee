// cluster_sites.hip.inc — the CpG-cluster stage from the per-position counters, on the device (part of summary.hip).
//
// Replaces, for one contig (or one rank's slice of it), the text round trip of the three tools after `detect`:
//   DeepMod_tools/sum_chr_mod.py:37-66          rows with mod > 0 of both strands, pct = int(mod * 100 / cov)
//   DeepMod_tools/generate_motif_pos.py:30-72   CpG hits: '+' at p where seq[p..p+1] == "CG", '-' at p + 1 (:62-63)
//   DeepMod_tools/hm_cluster_predict.py:43-72   readpredmod: rows on a motif position with coverage, frac = round(pct / 100, 3)
//   DeepMod_tools/hm_cluster_predict.py:128-154 the 14 features over the sites within +-25 bp
// deepmod_amd/cluster.py: sites_from_counters is the numpy twin of these kernels and the statement of the semantics.
//
// A position holds at most one site (a '+' site sits on a C, a '-' site on a G), so one byte per position says everything its neighbours
// need: 0 = no site, else (pct + 1) | strand << 7.  Three kernels, all O(length) bytes once:
//   site_code_kernel     code per position (sequence bytes + cov|mod of the strand the base belongs to) and the sites per tile and strand
//   site_scan_kernel     exclusive scan over [tiles of '+' | tiles of '-']: every site's output row follows from its position alone -
//                        '+' sites ascending, then '-' sites ascending, the order of the reference's file - and no atomic decides an order
//   site_feature_kernel  per tile: codes of tile +-26 in LDS, each site reads its 51 + partner codes, writes 14 fp32 features and its record
// The feature arithmetic is the reference's double arithmetic, operation for operation (divisions stay divisions, no contraction): the
// fp32 cast of the result is what the MLP is fed, and the file is compared byte for byte with the tools' (tests/test_gpu_cluster_fused.py).
#pragma once
#include "host.h"
#include "blockscan.hip.inc"

namespace csites {

constexpr int NB = 25;                  // hm_cluster_predict.py:83
constexpr int HALO = NB + 1;            // positions kept of either side of a range: the 25 a site at its edge reads (its partner lies among them) and one
                                        // of margin, the width the C ABI documents for the halo
constexpr int TILE = 1024;              // positions per block
constexpr int THREADS = 256;
constexpr int PER_THREAD = TILE / THREADS;
constexpr int SCAN_THREADS = 1024;

struct Args {
    const int* cov[2];                  // [0] '+', [1] '-': counters of positions first .. first + len[s] - 1 (nullptr: all zero)
    const int* mod[2];
    long long len[2];
    const int* halo;                    // [2 sides][2 strands][cov | mod][HALO]: positions first - 26 .. first - 1 and first + count .. + 25; nullptr: the table
    const int* tcov[2];                 // whole-table mode: the tables from position 0 (tlen[s] positions), read beside the range when no halo is given
    const int* tmod[2];
    long long tlen[2];
    const unsigned char* seq;           // bases of positions seq_first .. seq_first + seq_len - 1 (any case); outside: no base
    long long seq_first, seq_len;
    long long first, count;
};

__device__ inline int base_at(const Args& a, const long long q) {
    const long long j = q - a.seq_first;
    if (j < 0 || j >= a.seq_len) return 0;
    const int b = a.seq[j];
    return (b >= 'a' && b <= 'z') ? b - 32 : b;
}

// counters of strand s at index i relative to `first` (i in [-HALO, count + HALO))
__device__ inline void counts_at(const Args& a, const int s, const long long i, int& cv, int& md) {
    cv = 0;
    md = 0;
    if (i >= 0 && i < a.count) {
        if (a.cov[s] && i < a.len[s]) {
            cv = a.cov[s][i];
            md = a.mod[s][i];
        }
    } else if (a.halo) {
        const int side = i < 0 ? 0 : 1;
        const long long k = i < 0 ? i + HALO : i - a.count;
        if (k >= 0 && k < HALO) {
            const int* h = a.halo + ((side * 2 + s) * 2) * HALO;
            cv = h[k];
            md = h[HALO + k];
        }
    } else if (a.tcov[s]) {
        const long long q = a.first + i;
        if (q >= 0 && q < a.tlen[s]) {
            cv = a.tcov[s][q];
            md = a.tmod[s][q];
        }
    }
}

__device__ inline unsigned char site_code(const Args& a, const long long i) {
    const long long q = a.first + i;
    if (q < 0) return 0;
    const int b = base_at(a, q);
    int s;
    if (b == 'C') {
        if (base_at(a, q + 1) != 'G') return 0;
        s = 0;
    } else if (b == 'G') {
        if (base_at(a, q - 1) != 'C') return 0;
        s = 1;
    } else {
        return 0;
    }
    int cv, md;
    counts_at(a, s, i, cv, md);
    if (md <= 0 || cv <= 0) return 0;                        // sum_chr_mod.py:58 drops mod == 0; mod > 0 implies cov > 0 (dm_summary_add)
    const long long pct = (100ll * md) / cv;                  // int(mod * 100 / cov), sum_chr_mod.py:63
    return (unsigned char)((pct > 100 ? 100 : int(pct)) + 1) | (unsigned char)(s << 7);
}

__global__ __launch_bounds__(THREADS) void site_code_kernel(const Args a, unsigned char* __restrict__ code /* [count + 2 HALO] */,
                                                            int* __restrict__ bcount /* [2][nblocks] */, const long long nblocks) {
    __shared__ int cnt[2];
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * TILE;
    int n[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const long long i = t0 + k * THREADS + threadIdx.x;
        if (i < a.count) {
            const unsigned char c = site_code(a, i);
            code[i + HALO] = c;
            if (c) ++n[c >> 7];
        }
    }
    // the 26 positions on either side of the range: by the first and by the last block
    if (blockIdx.x == 0 && threadIdx.x < HALO) code[threadIdx.x] = site_code(a, (long long)threadIdx.x - HALO);
    if (blockIdx.x == nblocks - 1 && threadIdx.x >= HALO && threadIdx.x < 2 * HALO)
        code[a.count + threadIdx.x] = site_code(a, a.count + (threadIdx.x - HALO));
    if (n[0]) atomicAdd(&cnt[0], n[0]);                       // (a count: the order of the adds does not show)
    if (n[1]) atomicAdd(&cnt[1], n[1]);
    __syncthreads();
    if (threadIdx.x < 2) bcount[threadIdx.x * nblocks + blockIdx.x] = cnt[threadIdx.x];
}

// offs[i] = sum of bcount[0 .. i), i in [0, m]; one block walks the array (m = 2 x tiles: 5e5 values for a 2.5e8-position contig)
__global__ __launch_bounds__(SCAN_THREADS) void site_scan_kernel(const int* __restrict__ bcount, long long* __restrict__ offs, const long long m) {
    __shared__ long long wave_total[SCAN_THREADS / 64];
    long long carry = 0;
    for (long long base = 0; base < m; base += SCAN_THREADS) {
        const long long i = base + threadIdx.x;
        long long total;
        const long long ex = block_exclusive_scan<SCAN_THREADS>(i < m ? bcount[i] : 0, wave_total, total);
        if (i < m) offs[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) offs[m] = carry;
}

__device__ inline int bin_of_pct(const int pct) {
#pragma clang fp contract(off)
    const double frac = double(pct) / 100.0;                  // round(pct / 100.0, 3) is the identity on these (hm_cluster_predict.py:60)
    return int(frac / 0.1 + 0.5);                             // hm_cluster_predict.py:144
}

// the 14 features of the site at c[0]; c[-HALO .. HALO] are the codes around it
__device__ inline void site_features(const unsigned char* c, const unsigned char* bintab, float* f) {
#pragma clang fp contract(off)
    const int own = c[0];
    const int partner = (own >> 7) ? -1 : 1;                  // the C of the other strand in the same CpG
    f[0] = float(double((own & 127) - 1) / 100.0);
    const int pc = c[partner];
    f[1] = pc ? float(double((pc & 127) - 1) / 100.0) : 0.0f;
    unsigned long long lo = 0, hi = 0;                        // 11 counters of 8 bits (at most 50 neighbours): bins 0-5 | bins 6-10
    int n = 0;
    for (int d = -NB; d <= NB; ++d) {
        if (d == 0 || d == partner) continue;
        const int v = c[d];
        if (!v) continue;
        const int b = bintab[(v & 127) - 1];
        if (b < 6) lo += 1ull << (8 * b);
        else hi += 1ull << (8 * (b - 6));
        ++n;
    }
    f[2] = float(n);
#pragma unroll
    for (int b = 0; b < 11; ++b) {
        const int k = int(((b < 6 ? lo >> (8 * b) : hi >> (8 * (b - 6)))) & 255ull);
        // np.round(cnt / n, 3) = rint(x * 1000) / 1000 in double (hm_cluster_predict.py:150)
        f[3 + b] = n ? float(rint(double(k) / double(n) * 1000.0) / 1000.0) : 0.0f;
    }
}

__global__ __launch_bounds__(THREADS) void site_feature_kernel(const Args a, const unsigned char* __restrict__ code, const long long* __restrict__ offs,
                                                               const long long nblocks, float* __restrict__ feat, long long* __restrict__ rpos,
                                                               int* __restrict__ rcov, int* __restrict__ rmod) {
    __shared__ unsigned char lc[TILE + 2 * HALO];
    __shared__ unsigned char bintab[104];
    __shared__ long long wave_total[THREADS / 64];
    const long long t0 = (long long)blockIdx.x * TILE;
    const long long ecount = a.count + 2 * HALO;
    for (int j = threadIdx.x; j < TILE + 2 * HALO; j += THREADS) lc[j] = t0 + j < ecount ? code[t0 + j] : 0;
    if (threadIdx.x < 101) bintab[threadIdx.x] = (unsigned char)bin_of_pct(threadIdx.x);
    __syncthreads();
    // a thread owns PER_THREAD consecutive positions, so that the scan over the threads is the order of the positions
    const int j0 = threadIdx.x * PER_THREAD;
    long long mine = 0;                                       // '+' sites in the low word, '-' sites in the high word
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int c = t0 + j0 + k < a.count ? lc[HALO + j0 + k] : 0;
        if (c) mine += (c >> 7) ? (1ll << 32) : 1ll;
    }
    long long total;
    const long long ex = block_exclusive_scan<THREADS>(mine, wave_total, total);
    long long row[2] = {offs[blockIdx.x] + (ex & 0xffffffffll), offs[nblocks + blockIdx.x] + (ex >> 32)};
    for (int k = 0; k < PER_THREAD; ++k) {
        const long long i = t0 + j0 + k;
        if (i >= a.count) break;
        const unsigned char* c = lc + HALO + j0 + k;
        if (!*c) continue;
        const int s = *c >> 7;
        const long long r = row[s]++;
        float f[14];
        site_features(c, bintab, f);
        float2* o = reinterpret_cast<float2*>(feat + r * 14);    // 56-byte rows: 8-byte aligned
#pragma unroll
        for (int u = 0; u < 7; ++u) o[u] = make_float2(f[2 * u], f[2 * u + 1]);
        int cv, md;
        counts_at(a, s, i, cv, md);
        rpos[r] = a.first + i;
        rcov[r] = cv;
        rmod[r] = md;
    }
}

enum { B_SEQ, B_CODE, B_BCOUNT, B_OFFS, B_HALO, B_FEAT, B_POS, B_COV, B_MOD, B_PROB, B_COUNT };
static_assert(B_COUNT <= dm_cluster::SITE_BUFFERS, "dm_cluster holds one slot per buffer");

}  // namespace csites

extern "C" {

int64_t dm_cluster_sites(dm_cluster* c, dm_summary* plus, dm_summary* minus, int from_slice, const uint8_t* seq, int64_t seq_first, int64_t seq_len,
                         int64_t first, int64_t count, const int32_t* halo, int64_t* n_plus) {
    using namespace csites;
    if (!c) return fail(DM_EINVAL, "null cluster model");
    if (first < 0 || count < 0 || count > (int64_t(1) << 33) || seq_len < 0 || (seq_len > 0 && !seq))
        return fail(DM_EINVAL, "dm_cluster_sites: bad range (first %lld, count %lld, %lld bases)", (long long)first, (long long)count, (long long)seq_len);
    c->n_sites = c->n_plus = 0;
    if (n_plus) *n_plus = 0;
    Args a = {};
    a.seq_first = seq_first;
    a.seq_len = seq_len;
    a.first = first;
    a.count = count;
    dm_summary* both[2] = {plus, minus};
    HIP_TRY(hipSetDevice(c->device));
    for (int s = 0; s < 2; ++s) {
        dm_summary* t = both[s];
        if (!t) continue;
        if (t->device != c->device) return fail(DM_EINVAL, "summary on device %d, cluster model on device %d", t->device, c->device);
        if (t->follow) HIP_TRY(hipStreamSynchronize(model_stream(t->follow)));       // adds queued on the classifier's stream
        HIP_TRY(hipStreamSynchronize(t->stream));
        if (from_slice) {
            if (t->slice_count < 0) return fail(DM_ESTATE, "dm_cluster_sites: no reduce-scatter result in the '%c' summary", s ? '-' : '+');
            if (t->slice_first != first || t->slice_count != count)
                return fail(DM_EINVAL, "dm_cluster_sites: the '%c' summary holds the slice [%lld, +%lld), asked for [%lld, +%lld)", s ? '-' : '+',
                            (long long)t->slice_first, (long long)t->slice_count, (long long)first, (long long)count);
            a.cov[s] = t->slice() + t->slice_chunk;
            a.mod[s] = t->slice() + 2 * t->slice_chunk;
            a.len[s] = count;
        } else {
            a.len[s] = std::max<int64_t>(0, std::min<int64_t>(count, t->length - first));
            a.tcov[s] = t->d_counts + t->length;
            a.tmod[s] = t->d_counts + 2 * t->length;
            a.tlen[s] = t->length;
            if (a.len[s] > 0) {
                a.cov[s] = t->d_counts + t->length + first;
                a.mod[s] = t->d_counts + 2 * t->length + first;
            }
        }
    }
    if (count == 0 || seq_len == 0) return 0;
    const long long nblocks = (count + TILE - 1) / TILE;
    int rc;
    if ((rc = c->sites.ensure(B_SEQ, size_t(seq_len))) || (rc = c->sites.ensure(B_CODE, size_t(count) + 2 * HALO)) ||
        (rc = c->sites.ensure(B_BCOUNT, sizeof(int) * 2 * size_t(nblocks))) || (rc = c->sites.ensure(B_OFFS, sizeof(long long) * (2 * size_t(nblocks) + 1))) ||
        (rc = c->sites.ensure(B_HALO, sizeof(int) * 8 * HALO)))
        return rc;
    HIP_TRY(hipMemcpyAsync(c->sites.buf[B_SEQ], seq, size_t(seq_len), hipMemcpyHostToDevice, c->stream));
    a.seq = static_cast<const unsigned char*>(c->sites.buf[B_SEQ]);
    if (halo) {
        HIP_TRY(hipMemcpyAsync(c->sites.buf[B_HALO], halo, sizeof(int) * 8 * HALO, hipMemcpyHostToDevice, c->stream));
        a.halo = static_cast<const int*>(c->sites.buf[B_HALO]);
    }
    unsigned char* d_code = static_cast<unsigned char*>(c->sites.buf[B_CODE]);
    int* d_bcount = static_cast<int*>(c->sites.buf[B_BCOUNT]);
    long long* d_offs = static_cast<long long*>(c->sites.buf[B_OFFS]);
    hipLaunchKernelGGL(site_code_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, c->stream, a, d_code, d_bcount, nblocks);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(site_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, c->stream, d_bcount, d_offs, 2 * nblocks);
    HIP_TRY(hipGetLastError());
    long long totals[2] = {0, 0};                             // '+' sites, all sites
    HIP_TRY(hipMemcpyAsync(&totals[0], d_offs + nblocks, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&totals[1], d_offs + 2 * nblocks, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const long long n = totals[1];
    if (n < 0 || totals[0] < 0 || totals[0] > n || n > count) return fail(DM_EDEVICE, "dm_cluster_sites: inconsistent site counts (%lld, %lld)", totals[0], n);
    if (n == 0) return 0;
    if ((rc = c->sites.ensure(B_FEAT, sizeof(float) * 14 * size_t(n))) || (rc = c->sites.ensure(B_POS, sizeof(long long) * size_t(n))) ||
        (rc = c->sites.ensure(B_COV, sizeof(int) * size_t(n))) || (rc = c->sites.ensure(B_MOD, sizeof(int) * size_t(n))) || (rc = c->sites.ensure(B_PROB, sizeof(float) * size_t(n))))
        return rc;
    float* d_feat = static_cast<float*>(c->sites.buf[B_FEAT]);
    hipLaunchKernelGGL(site_feature_kernel, dim3((unsigned)nblocks), dim3(THREADS), 0, c->stream, a, d_code, d_offs, nblocks, d_feat,
                       static_cast<long long*>(c->sites.buf[B_POS]), static_cast<int*>(c->sites.buf[B_COV]), static_cast<int*>(c->sites.buf[B_MOD]));
    HIP_TRY(hipGetLastError());
    // the MLP of dm_cluster_predict, on the feature rows where they are
    const int blocks = int(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(cluster_mlp_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_w, d_feat, n, static_cast<float*>(c->sites.buf[B_PROB]));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n_sites = n;
    c->n_plus = totals[0];
    if (n_plus) *n_plus = totals[0];
    return n;
}

int dm_cluster_sites_fetch(dm_cluster* c, int64_t* pos, int32_t* cov, int32_t* mod, int32_t* new_pct, float* features) {
    using namespace csites;
    if (!c) return fail(DM_EINVAL, "null cluster model");
    const size_t n = size_t(c->n_sites);
    if (n == 0) return DM_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (pos) HIP_TRY(hipMemcpy(pos, c->sites.buf[B_POS], sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    if (cov) HIP_TRY(hipMemcpy(cov, c->sites.buf[B_COV], sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (mod) HIP_TRY(hipMemcpy(mod, c->sites.buf[B_MOD], sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (features) HIP_TRY(hipMemcpy(features, c->sites.buf[B_FEAT], sizeof(float) * 14 * n, hipMemcpyDeviceToHost));
    if (new_pct) {
        std::vector<float> p(n);
        HIP_TRY(hipMemcpy(p.data(), c->sites.buf[B_PROB], sizeof(float) * n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) new_pct[i] = int32_t(p[i] * 100.0f);      // int(float32 p * 100), hm_cluster_predict.py:170
    }
    return DM_OK;
}

}  // extern "C"
