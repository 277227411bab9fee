// motifs.inc — `motifs`: the rule of a key, the compiled host twin, and (under hipcc) the handle and the C ABI.  The first part is plain C++: part of
// offline.hip, and compiled by g++ as it stands (tests/motifs_asan_driver.cpp).  The kernels of motifs.hip.inc and dm_motifs_count_host run the
// same routine (mok::fate), so the device and the host cannot disagree on a key.  deepmod_amd/motifs.py (HostEngine) states the semantics in numpy;
// DESIGN.md 20.
//
// One contig: its bytes as handed over (no case folding), the sample's '+' and '-' tables (coverage, modified count per position) and optionally the
// pooled controls' tables.  Each key (strand s, position p) is examined once; the first rule that applies decides (mok::fate):
//   1  the oriented letter (seq[p] on '+', its complement on '-') is not `base`: off_base if the sample's coverage is > 0, else ignored
//   2  the oriented context, offsets -U..-1 and +1..+D ('+': seq[p + j]; '-': the complement of seq[p - j]), leaves the contig or holds a byte other
//      than A, C, G, T: edge
//   3  sample coverage < cov: shallow            4  controls given and their coverage < cov: no_control
//   5  tested; modified too if 100 mod >= min_pct cov and (no controls or 100 cmod < (max_ctrl_pct + 1) ccov)
// which are 100 mod // cov >= min_pct and 100 cmod // ccov <= max_ctrl_pct for cov, ccov >= 1, in 64-bit products: exact for every int32 count.
// The context index has its most significant base-4 digit at offset -U, A < C < G < T.
// Two guarded parts, so that this file and motifs.hip.inc can be included in either order: the rule, which the kernels include, and the handle, which
// includes the kernels.
#ifndef DM_MOTIFS_RULE_INC
#define DM_MOTIFS_RULE_INC
#ifdef __HIP__
#include "host.h"
#endif
#include "bedline.inc"
#include "../../include/deepmod_hip.h"

namespace mok {

constexpr long long MAX_LENGTH = 0x7fffffffLL;      // positions of a contig, 1 to 2^31 - 1 (the tables are int32-indexed text positions)
constexpr int MAX_FLANK = 8;                        // U, D and U + D
constexpr int TILE_POS = 1024;                      // positions of one tile of the sweep (dm_motifs_tile_positions)
constexpr int LDS_FLANK = 6;                        // U + D <= 6: 4^6 bins x 2 columns x 4 bytes = 32 KB, a workgroup counts in LDS; above: in global memory
constexpr unsigned BAD = 4u;                        // the validity bit of a code byte: outside the contig, or none of A, C, G, T
enum { K_TESTED, K_MODIFIED, K_SHALLOW, K_NOCTRL, K_EDGE, N_COUNT };           // the counters of a strand
enum { F_IGNORED = -2, F_OFF_BASE = -1, F_TESTED = K_TESTED, F_MODIFIED = K_MODIFIED, F_SHALLOW = K_SHALLOW, F_NOCTRL = K_NOCTRL, F_EDGE = K_EDGE };

struct Rule {
    int up, down, cov, min_pct, max_ctrl_pct;
    unsigned base;                                  // the 2-bit code of --Base
};

// A 0, C 1, G 2, T 3 (upper case only: the engine does not fold case), anything else BAD; the complement of code c is 3 - c
BED_HD inline unsigned code_of(const unsigned char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : BAD; }

inline long long bins_of(const int up, const int down) { return 1LL << (2 * (up + down)); }

// null: the options are in range; else what is wrong with them
inline const char* check_rule(const int up, const int down, const char base, const int cov, const int min_pct, const int max_ctrl_pct) {
    if (up < 0 || down < 0 || up > MAX_FLANK || down > MAX_FLANK || up + down > MAX_FLANK) return "a flank of 0 to 8 bases on either side, 8 in all at most";
    if (code_of((unsigned char)base) == BAD) return "a base of A, C, G, T";
    if (cov < 1) return "a least coverage of 1 or more";
    if (min_pct < 0 || min_pct > 100) return "a least percentage of 0 to 100";
    if (max_ctrl_pct < 0 || max_ctrl_pct > 100) return "a largest control percentage of 0 to 100";
    return nullptr;
}

// The fate of key (s, p): F_*.  at(q): the code byte of position q, BAD outside the contig.  ctx: the context index of a key that is F_TESTED or
// F_MODIFIED.  cv, md: the sample's counters at p; ctrl: controls are given, ccv, cmd: theirs.
template <class Codes>
BED_HD inline int fate(const Codes& at, const long long p, const int s, const Rule& r, const int cv, const int md, const bool ctrl, const int ccv, const int cmd,
                       unsigned& ctx) {
    const unsigned own = at(p);
    if (own != (s ? 3u - r.base : r.base)) return cv > 0 ? F_OFF_BASE : F_IGNORED;
    unsigned c = 0, bad = 0;
    for (int j = -r.up; j <= r.down; ++j) {
        if (j == 0) continue;
        const unsigned v = at(s ? p - j : p + j);
        bad |= v;
        c = c * 4u + (s ? 3u - (v & 3u) : (v & 3u));
    }
    if (bad & BAD) return F_EDGE;
    if (cv < r.cov) return F_SHALLOW;
    if (ctrl && ccv < r.cov) return F_NOCTRL;
    ctx = c;
    const bool high = 100LL * md >= (long long)r.min_pct * cv;
    const bool quiet = !ctrl || 100LL * cmd < (long long)(r.max_ctrl_pct + 1) * ccv;
    return high && quiet ? F_MODIFIED : F_TESTED;
}

struct HostCodes {
    const unsigned char* seq;
    long long len;
    unsigned operator()(const long long q) const { return q < 0 || q >= len ? BAD : code_of(seq[q]); }
};

// The sweep on the host, one key after the other: hist [4^(U+D)][2] +=, counters [2][N_COUNT] and off_base [2] = those of this contig.
// tab[s][0 / 1]: coverage / modified of strand s; ctl: the same of the controls, or null.
inline void count_host(const Rule& r, const unsigned char* seq, const long long len, const int32_t* const tab[2][2], const int32_t* const (*ctl)[2], int64_t* hist,
                       int64_t* counters, int64_t* off_base) {
    for (int j = 0; j < 2 * N_COUNT; ++j) counters[j] = 0;
    off_base[0] = off_base[1] = 0;
    const HostCodes at = {seq, len};
    for (long long p = 0; p < len; ++p)
        for (int s = 0; s < 2; ++s) {
            unsigned ctx = 0;
            const int f = fate(at, p, s, r, tab[s][0][p], tab[s][1][p], ctl != nullptr, ctl ? ctl[s][0][p] : 0, ctl ? ctl[s][1][p] : 0, ctx);
            if (f == F_IGNORED) continue;
            if (f == F_OFF_BASE) {
                ++off_base[s];
                continue;
            }
            ++counters[s * N_COUNT + (f == F_MODIFIED ? int(K_TESTED) : f)];
            if (f == F_TESTED || f == F_MODIFIED) ++hist[2 * (long long)ctx];
            if (f == F_MODIFIED) {
                ++counters[s * N_COUNT + K_MODIFIED];
                ++hist[2 * (long long)ctx + 1];
            }
        }
}

}  // namespace mok

#ifdef __HIP__
#define MOK_FAIL(...) fail(DM_EINVAL, __VA_ARGS__)
#else
#define MOK_FAIL(...) DM_EINVAL
#endif

// The compiled host twin of the sweep (no GPU needed): a contig of len >= 0 positions, every table of len entries; the four control tables all given
// or all null.  hist [4^(up+down)][2] is added to, counters [2][5] and off_base [2] are set.
extern "C" int dm_motifs_count_host(int up, int down, char base, int cov, int min_pct, int max_ctrl_pct, const uint8_t* seq, int64_t len, const int32_t* cov_plus,
                                    const int32_t* mod_plus, const int32_t* cov_minus, const int32_t* mod_minus, const int32_t* ctrl_cov_plus, const int32_t* ctrl_mod_plus,
                                    const int32_t* ctrl_cov_minus, const int32_t* ctrl_mod_minus, int64_t* hist, int64_t* counters, int64_t* off_base) {
    const char* why = mok::check_rule(up, down, base, cov, min_pct, max_ctrl_pct);
    if (why) return MOK_FAIL("dm_motifs_count_host: %s", why);
    if (len < 0 || len > mok::MAX_LENGTH) return MOK_FAIL("dm_motifs_count_host: a contig of %lld positions (0 to 2^31 - 1)", (long long)len);
    if (!hist || !counters || !off_base || (len > 0 && (!seq || !cov_plus || !mod_plus || !cov_minus || !mod_minus))) return MOK_FAIL("dm_motifs_count_host: null argument");
    const int given = (ctrl_cov_plus != nullptr) + (ctrl_mod_plus != nullptr) + (ctrl_cov_minus != nullptr) + (ctrl_mod_minus != nullptr);
    if (given != 0 && given != 4) return MOK_FAIL("dm_motifs_count_host: the controls are given by all four of their tables or by none");
    const mok::Rule r = {up, down, cov, min_pct, max_ctrl_pct, mok::code_of((unsigned char)base)};
    const int32_t* const tab[2][2] = {{cov_plus, mod_plus}, {cov_minus, mod_minus}};
    const int32_t* const ctl[2][2] = {{ctrl_cov_plus, ctrl_mod_plus}, {ctrl_cov_minus, ctrl_mod_minus}};
    mok::count_host(r, seq, len, tab, given ? ctl : nullptr, hist, counters, off_base);
    return DM_OK;
}

#endif  // DM_MOTIFS_RULE_INC

#if defined(__HIP__) && !defined(DM_MOTIFS_HANDLE_INC) && !defined(DM_MOTIFS_RULE_ONLY)
#define DM_MOTIFS_HANDLE_INC
#include "motifs.hip.inc"
#include "tablestage.hip.inc"

struct dm_motifs_buf {
    enum { SEQ, HIST, COUNTS, N_BUF };
};
struct dm_motifs : dm_motifs_buf, TableStage<4, dm_motifs_buf::N_BUF> {       // events: upload, count: begin / end
    mok::Rule rule = {};
    long long bins = 0;
    double upload_ms = 0.0, count_ms = 0.0;
};

extern "C" {

int dm_motifs_tile_positions(void) { return mok::TILE_POS; }

void dm_motifs_destroy(dm_motifs* h) {
    if (!h) return;
    h->shut();
    delete h;
}

dm_motifs* dm_motifs_create(int device, int up, int down, char base, int cov, int min_pct, int max_ctrl_pct) {
    const char* why = mok::check_rule(up, down, base, cov, min_pct, max_ctrl_pct);
    if (why) {
        fail(DM_EINVAL, "dm_motifs_create: %s (got flank %d,%d base 0x%02x cov %d min_pct %d max_ctrl_pct %d)", why, up, down, (unsigned)(unsigned char)base, cov, min_pct,
             max_ctrl_pct);
        return nullptr;
    }
    if (!table_stage_device("dm_motifs", device)) return nullptr;
    dm_motifs* h = new dm_motifs;
    h->rule = {up, down, cov, min_pct, max_ctrl_pct, mok::code_of((unsigned char)base)};
    h->bins = mok::bins_of(up, down);
    bool ok = h->open(device, "dm_motifs");
    ok = ok && h->b.ensure(dm_motifs::HIST, size_t(h->bins) * 16) == DM_OK && h->b.ensure(dm_motifs::COUNTS, mok::N_SWEEP * 8) == DM_OK;
    ok = ok && h->zero_block(dm_motifs::HIST, size_t(h->bins) * 16) == DM_OK;
    if (!ok) {
        (void)hipGetLastError();
        fail(DM_EDEVICE, "dm_motifs_create: stream, events or counters on device %d", device);
        dm_motifs_destroy(h);
        return nullptr;
    }
    return h;
}

int dm_motifs_count(dm_motifs* h, const uint8_t* seq, int64_t len, dm_summary* plus, dm_summary* minus, dm_summary* ctrl_plus, dm_summary* ctrl_minus, int64_t* counters,
                    int64_t* off_base) {
    using B = dm_motifs;
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!seq || !counters || !off_base) return fail(DM_EINVAL, "dm_motifs_count: null argument");
    if (!plus || !minus || plus == minus) return fail(DM_EINVAL, "dm_motifs_count: two sample tables, one per strand (null handle)");
    if ((ctrl_plus == nullptr) != (ctrl_minus == nullptr)) return fail(DM_EINVAL, "dm_motifs_count: the controls are given by both of their tables or by neither");
    if (ctrl_plus && (ctrl_plus == ctrl_minus || ctrl_plus == plus || ctrl_plus == minus || ctrl_minus == plus || ctrl_minus == minus))
        return fail(DM_EINVAL, "dm_motifs_count: the control tables are two tables of their own");
    if (len < 1 || len > mok::MAX_LENGTH) return fail(DM_EINVAL, "dm_motifs_count: a contig of %lld positions (1 to 2^31 - 1)", (long long)len);
    dm_summary* tab[4] = {plus, minus, ctrl_plus, ctrl_minus};
    const int n_tab = ctrl_plus ? 4 : 2;
    for (int j = 0; j < n_tab; ++j)
        if (dm_summary_length(tab[j]) != len)
            return fail(DM_EINVAL, "dm_motifs_count: table %d has %lld positions, the contig %lld", j, (long long)dm_summary_length(tab[j]), (long long)len);
    int rc;
    if ((rc = h->tables_ready("dm_motifs_count", tab, n_tab)) != DM_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = h->b.ensure(B::SEQ, size_t(len))) != DM_OK) return rc;
    hipStream_t s = h->stream;
    unsigned long long* d_counts = h->b.ptr<unsigned long long>(B::COUNTS);
    HIP_TRY(hipEventRecord(h->ev[0], s));
    HIP_TRY(hipMemcpyAsync(h->b.buf[B::SEQ], seq, size_t(len), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(h->ev[1], s));
    HIP_TRY(hipMemsetAsync(d_counts, 0, mok::N_SWEEP * 8, s));
    const long long tiles = (len + mok::TILE_POS - 1) / mok::TILE_POS;
    const dim3 grid{unsigned(std::min<long long>(tiles, mok::MAX_BLOCKS))};
    const int* t[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; j < n_tab; ++j) t[j] = static_cast<const int*>(dm_summary_device_ptr(tab[j]));
    HIP_TRY(hipEventRecord(h->ev[2], s));
    if (h->rule.up + h->rule.down <= mok::LDS_FLANK)
        hipLaunchKernelGGL(mok::mo_count_kernel<true>, grid, dim3(mok::THREADS), 0, s, h->b.ptr<const unsigned char>(B::SEQ), (long long)len, t[0], t[1], t[2], t[3], h->rule,
                           h->b.ptr<unsigned long long>(B::HIST), d_counts);
    else
        hipLaunchKernelGGL(mok::mo_count_kernel<false>, grid, dim3(mok::THREADS), 0, s, h->b.ptr<const unsigned char>(B::SEQ), (long long)len, t[0], t[1], t[2], t[3], h->rule,
                           h->b.ptr<unsigned long long>(B::HIST), d_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev[3], s));
    long long got[mok::N_SWEEP] = {};
    HIP_TRY(hipMemcpyAsync(got, d_counts, sizeof got, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                                 // the caller's bytes are read by now
    if ((rc = add_time(h->ev[0], h->ev[1], h->upload_ms)) != DM_OK || (rc = add_time(h->ev[2], h->ev[3], h->count_ms)) != DM_OK) return rc;
    for (int j = 0; j < 2 * mok::N_COUNT; ++j) counters[j] = got[j];
    off_base[0] = got[2 * mok::N_COUNT];
    off_base[1] = got[2 * mok::N_COUNT + 1];
    return DM_OK;
}

int dm_motifs_fetch(dm_motifs* h, int64_t* hist) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (!hist) return fail(DM_EINVAL, "dm_motifs_fetch: null argument");
    return h->fetch_block(dm_motifs::HIST, hist, size_t(h->bins) * 16);
}

int dm_motifs_reset(dm_motifs* h) {
    if (!h) return fail(DM_EINVAL, "null handle");
    return h->zero_block(dm_motifs::HIST, size_t(h->bins) * 16);
}

int dm_motifs_times(dm_motifs* h, double* upload_ms, double* count_ms) {
    if (!h) return fail(DM_EINVAL, "null handle");
    if (upload_ms) *upload_ms = h->upload_ms;
    if (count_ms) *count_ms = h->count_ms;
    return DM_OK;
}

}  // extern "C"
#endif  // the handle
