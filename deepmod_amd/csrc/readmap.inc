// readmap.inc — SAM record + reference sequence -> per-base alignment table (host C++, part of feed.hip).
//
// Replaces the alignment walk of handle_record, /root/reference/bin/DeepMod_scripts/myDetect.py:515-714:
//   :515-520  POS -> 0-based, strand from FLAG 0x10, CIGAR split into counts and ops
//   :522-536  strip leading / trailing I D N S H P X operations into leftclip / rightclip (I, S, X consume read
//             bases; D, N, X on the left advance the reference position)
//   :537-542  the event slice that remains for the strand
//   :558-616  one table row (refbase, readbase, refpos, readpos) per M / I / D / N / = / X position; first / last
//             matching base (read index, row index, reference position); mismatch / insertion / deletion counts
//   :617-622  no matching base at all -> the read is skipped
//   :624-644  unmatched ends are added to the clips and cut from the event slice
//   :645-659  the table is cut to [first matching row, last matching row]
//   :661-667  '-' strand: table reversed, both bases complemented (A C G T a c g t N n), clips swapped
//   :684-704  the CpG special case: "C -...- G" against reference "C G...G G" (and its mirror image) swaps the gap
// This is sequential, branchy byte work on one read (10^3 - 10^5 rows) — it stays on the host, as in the reference,
// but as compiled code instead of a per-base Python loop.
#pragma once
#include "host.h"

namespace readmap {

struct ComplementTable {
    unsigned char t[256];
    constexpr ComplementTable() : t() {
        for (int i = 0; i < 256; ++i) t[i] = static_cast<unsigned char>(i);   // 'N', 'n' map to themselves, everything else ('-') is left alone
        t['A'] = 'T'; t['C'] = 'G'; t['G'] = 'C'; t['T'] = 'A';
        t['a'] = 't'; t['c'] = 'g'; t['g'] = 'c'; t['t'] = 'a';
    }
};
constexpr ComplementTable kComplement{};
inline char complement(char c) { return char(kComplement.t[static_cast<unsigned char>(c)]); }

// small runs dominate a nanopore CIGAR (a dozen positions between two indels): a call of memcpy / memset per run costs more than the bytes
inline void copy_run(char* dst, const char* src, int64_t n) {
    if (n >= 32) std::memcpy(dst, src, size_t(n));
    else
        for (int64_t j = 0; j < n; ++j) dst[j] = src[j];
}
inline void fill_run(char* dst, char c, int64_t n) {
    if (n >= 32) std::memset(dst, c, size_t(n));
    else
        for (int64_t j = 0; j < n; ++j) dst[j] = c;
}

inline bool is_clip_op(char op) { return op == 'I' || op == 'D' || op == 'N' || op == 'S' || op == 'H' || op == 'P' || op == 'X'; }

// The walk of :558-616 written STRAIGHT into the caller's columns (forward order, untrimmed; round 6 - rounds 1-5 pushed 24-byte row records into a
// vector and copied them out column by column), then the clip / event-slice arithmetic of :624-644, the cut to the matching rows (:645-659), the
// '-' strand flip with complement (:661-667) and the CpG gap swap (:684-704), all in place.  Runs of M / = / X / I / D / N are bounds-checked once
// per run and written with memcpy / memset + an index ramp.
//   cap        rows the columns hold.  The untrimmed table needs *need_rows (always set once the CIGAR is parsed): with cap < *need_rows nothing is
//              written and info[DM_MAP_STATUS] = DM_MAP_NEED_ROWS.
//   readi      may be NULL (the streaming row builder never reads the read-index column)
//   first_row  the final table is rows [*first_row, *first_row + info[DM_MAP_N_ROWS]) of the columns
// Declared in host.h (cpg_swap defaults to true there): getfeatures calls it from another translation unit.
int map_read_core(int flag, int64_t pos1, const char* cigar, const char* readseq, int64_t readseq_len, const char* refseq, int64_t refseq_len,
                  int64_t n_events, char* refb, char* readb, int64_t* refi, uint64_t* readi, int64_t cap, int64_t* info, int64_t* first_row,
                  int64_t* need_rows, const bool cpg_swap) {
    for (int i = 0; i < DM_MAP_INFO_LEN; ++i) info[i] = 0;
    *first_row = 0;
    *need_rows = 0;
    // ---- CIGAR -> (count, op) lists: digit runs and [MIDNSHPX=] characters, like the two regexes of :497-498 ----
    // (scratch of this thread, bound to locals once: in a shared library every mention of a thread_local is a call of __tls_get_addr)
    thread_local std::vector<int64_t> tl_num;
    thread_local std::vector<char> tl_ops;
    std::vector<int64_t>& num = tl_num;
    std::vector<char>& ops = tl_ops;
    num.clear();
    ops.clear();
    {
        int64_t cur = -1;
        for (const char* p = cigar; *p; ++p) {
            const char ch = *p;
            if (ch >= '0' && ch <= '9') {
                cur = (cur < 0 ? 0 : cur) * 10 + (ch - '0');
                if (cur > (int64_t(1) << 40)) return fail(DM_EINVAL, "dm_map_read: a CIGAR count beyond 2^40");
            } else {
                if (cur >= 0) num.push_back(cur);
                cur = -1;
                if (std::strchr("MIDNSHPX=", ch)) ops.push_back(ch);
            }
        }
        if (cur >= 0) num.push_back(cur);
    }
    if (ops.empty() || num.size() != ops.size()) return fail(DM_EINVAL, "dm_map_read: malformed CIGAR '%s'", cigar);

    int64_t pos = pos1 - 1;
    const bool reverse = (flag & 0x10) != 0;
    int64_t leftclip = 0, rightclip = 0;
    int64_t seq_lo = 0, seq_hi = readseq_len;       // readseq[seq_lo:seq_hi] is what is left of the read
    size_t first_op = 0, end_op = ops.size();
    while (first_op < end_op && is_clip_op(ops[first_op])) {
        const char op = ops[first_op];
        const int64_t n = num[first_op];
        if (op == 'I' || op == 'S' || op == 'X') {
            leftclip += n;
            seq_lo += n;
        }
        if (op == 'H') leftclip += n;
        if (op == 'D' || op == 'N' || op == 'X') pos += n;
        ++first_op;
    }
    if (first_op == end_op) return fail(DM_EINVAL, "dm_map_read: CIGAR '%s' has no aligned segment", cigar);
    while (end_op > first_op && is_clip_op(ops[end_op - 1])) {
        const char op = ops[end_op - 1];
        const int64_t n = num[end_op - 1];
        if (op == 'I' || op == 'S' || op == 'X') {
            rightclip += n;
            seq_hi -= n;
        }
        if (op == 'H') rightclip += n;
        --end_op;
    }
    if (seq_lo > readseq_len) seq_lo = readseq_len;             // python slices clamp
    if (seq_hi < seq_lo) seq_hi = seq_lo;
    const char* seq = readseq + seq_lo;
    const int64_t seq_len = seq_hi - seq_lo;

    // events left after removing the clipped bases (python slice arithmetic on a list of n_events items)
    auto clamp = [&](int64_t v) { return v < 0 ? 0 : (v > n_events ? n_events : v); };
    int64_t ev_lo, ev_hi;
    if (!reverse) {
        ev_lo = clamp(leftclip);
        ev_hi = rightclip > 0 ? clamp(n_events - rightclip) : n_events;
    } else {
        ev_lo = clamp(rightclip);
        ev_hi = leftclip > 0 ? clamp(n_events - leftclip) : n_events;
    }
    if (ev_hi < ev_lo) ev_hi = ev_lo;
    int64_t n_ev = ev_hi - ev_lo;
    info[DM_MAP_POS_AFTER_CLIP] = pos;
    info[DM_MAP_EVENTS_AFTER_CLIP] = n_ev;

    // ---- rows of the untrimmed table: every M / = / X / I / D / N position ----
    int64_t total = 0;
    for (size_t k = first_op; k < end_op; ++k)
        if (ops[k] != 'S' && ops[k] != 'H' && ops[k] != 'P') total += num[k];       // (counts are <= 2^40 each and a CIGAR has < 2^20 of them)
    *need_rows = total;
    // every table row consumes a read base or a reference base: a CIGAR that claims more runs past one of them - walked without writing for its error
    const bool write = total <= cap && total <= readseq_len + refseq_len + 16 && refb && readb && refi;
    if (!write && total <= readseq_len + refseq_len + 16) {
        info[DM_MAP_STATUS] = DM_MAP_NEED_ROWS;
        info[DM_MAP_N_ROWS] = total;
        return DM_OK;
    }

    // ---- walk (:558-616) ----
    bool have_match = false;
    int64_t firstmatch = -1, lastmatch = -1, first_al = -1, last_al = -1, first_pos = -1, last_pos = -1;
    int64_t nummismatch = 0, numinsert = 0, numdel = 0, read_ind = 0, nrow = 0;
    for (size_t k = first_op; k < end_op; ++k) {
        const char op = ops[k];
        const int64_t n = num[k];
        if (op == 'S') {               // soft clip in the middle of the alignment: the reference only warns
            read_ind += n;
            continue;
        }
        if (op == 'H' || op == 'P') continue;      // in the middle: nothing
        if (op == 'M' || op == '=' || op == 'X') {
            if (pos < 0 || read_ind < 0 || n > refseq_len - pos || n > seq_len - read_ind) {
                const int64_t jr = pos < 0 ? 0 : std::max<int64_t>(0, refseq_len - pos), jq = read_ind < 0 ? 0 : std::max<int64_t>(0, seq_len - read_ind);
                const int64_t j = std::min(jr, jq);
                return fail(DM_EINVAL, "dm_map_read: CIGAR runs past the %s (pos %lld, read index %lld)", pos + j >= refseq_len ? "reference" : "read",
                            (long long)(pos + j), (long long)(read_ind + j));
            }
            const char* rp = refseq + pos;
            const char* qp = seq + read_ind;
            if (write) {
                copy_run(refb + nrow, rp, n);
                copy_run(readb + nrow, qp, n);
                for (int64_t j = 0; j < n; ++j) refi[nrow + j] = pos + j;
                if (readi)
                    for (int64_t j = 0; j < n; ++j) readi[nrow + j] = uint64_t(read_ind + j);
            }
            int64_t jf = -1, jl = -1;              // first / last matching position of the run
            if (op == '=') {
                if (n > 0) {
                    jf = 0;
                    jl = n - 1;
                }
            } else if (op == 'M') {
                int64_t mism = 0;                  // three plain loops: the count vectorises, the two searches end at once on a typical run
                for (int64_t j = 0; j < n; ++j) mism += rp[j] != qp[j];
                nummismatch += mism;
                if (mism < n) {
                    jf = 0;
                    while (rp[jf] != qp[jf]) ++jf;
                    jl = n - 1;
                    while (rp[jl] != qp[jl]) --jl;
                }
            } else {
                nummismatch += n;
            }
            if (jf >= 0) {
                if (!have_match) {
                    firstmatch = read_ind + jf;
                    first_al = nrow + jf;
                    first_pos = pos + jf;
                    have_match = true;
                }
                lastmatch = read_ind + jl;
                last_al = nrow + jl;
                last_pos = pos + jl;
            }
            pos += n;
            read_ind += n;
            nrow += n;
        } else if (op == 'I') {
            if (read_ind < 0 || n > seq_len - read_ind) return fail(DM_EINVAL, "dm_map_read: CIGAR runs past the read");
            if (write) {
                fill_run(refb + nrow, '-', n);
                copy_run(readb + nrow, seq + read_ind, n);
                for (int64_t j = 0; j < n; ++j) refi[nrow + j] = pos;
                if (readi)
                    for (int64_t j = 0; j < n; ++j) readi[nrow + j] = uint64_t(read_ind + j);
            }
            read_ind += n;
            numinsert += n;
            nrow += n;
        } else {                       // 'D' or 'N'
            if (pos < 0 || n > refseq_len - pos) return fail(DM_EINVAL, "dm_map_read: CIGAR runs past the reference");
            if (write) {
                copy_run(refb + nrow, refseq + pos, n);
                fill_run(readb + nrow, '-', n);
                for (int64_t j = 0; j < n; ++j) refi[nrow + j] = pos + j;
                if (readi)
                    for (int64_t j = 0; j < n; ++j) readi[nrow + j] = uint64_t(read_ind);
            }
            pos += n;
            if (op == 'D') numdel += n;
            nrow += n;
        }
    }
    if (!write) return fail(DM_EINVAL, "dm_map_read: a CIGAR of %lld positions for a read of %lld and a reference of %lld bases", (long long)total,
                            (long long)readseq_len, (long long)refseq_len);
    info[DM_MAP_NUM_INSERT] = numinsert;
    info[DM_MAP_NUM_DELETE] = numdel;
    info[DM_MAP_NUM_MISMATCH] = nummismatch;
    info[DM_MAP_STRAND] = reverse ? 1 : 0;
    if (!have_match) {
        info[DM_MAP_STATUS] = DM_MAP_NO_MATCH;     // :617-622: read skipped
        return DM_OK;
    }
    // ---- unmatched ends -> clips, event slice (:624-644) ----
    const int64_t tail = n_ev - lastmatch;          // len(m_event) - lastmatch
    if (!reverse) {
        leftclip += firstmatch;
        if (tail > 1) rightclip += tail - 1;
    } else {
        rightclip += firstmatch;
        if (tail > 1) leftclip += tail - 1;
    }
    {
        // python: m_event[a:b] on a list of n_ev items, negative b counts from the end
        auto slice = [&](int64_t a, bool has_b, int64_t b) {
            if (a < 0) a = std::max<int64_t>(0, n_ev + a);
            if (a > n_ev) a = n_ev;
            int64_t e = n_ev;
            if (has_b) {
                e = b < 0 ? std::max<int64_t>(0, n_ev + b) : std::min<int64_t>(b, n_ev);
            }
            if (e < a) e = a;
            ev_hi = ev_lo + e;
            ev_lo = ev_lo + a;
            n_ev = e - a;
        };
        if (!reverse) {
            if (tail > 1) slice(firstmatch, true, lastmatch + 1 - n_ev);
            else if (firstmatch > 0) slice(firstmatch, false, 0);
        } else {
            if (firstmatch > 0) slice(n_ev - 1 - lastmatch, true, -firstmatch);
            else if (tail > 1) slice(n_ev - 1 - lastmatch, false, 0);
        }
    }
    // ---- table cut to the matching rows (:645-659) ----
    int64_t r0 = 0, r1 = nrow;
    if (firstmatch > 0 || nrow - last_al > 1) {
        if (nrow - last_al > 1) {
            r0 = first_al;
            r1 = last_al + 1;
        } else if (first_al > 0) {
            r0 = first_al;
        }
    }
    const int64_t n_rows = r1 - r0;
    info[DM_MAP_N_ROWS] = n_rows;
    info[DM_MAP_FIRST_MATCH_POS] = first_pos;
    info[DM_MAP_LAST_MATCH_POS] = last_pos;
    info[DM_MAP_EV_LO] = ev_lo;
    info[DM_MAP_EV_HI] = ev_hi;
    *first_row = r0;
    char* const tb = refb + r0;
    char* const qb = readb + r0;
    if (reverse) {                     // :661-667: table reversed, both bases complemented, clips swapped
        int64_t* const ti = refi + r0;
        for (int64_t a = 0, b = n_rows - 1; a <= b; ++a, --b) {
            const char ta = complement(tb[a]), tbb = complement(tb[b]), qa = complement(qb[a]), qbb = complement(qb[b]);
            tb[a] = tbb;
            tb[b] = ta;
            qb[a] = qbb;
            qb[b] = qa;
            std::swap(ti[a], ti[b]);
        }
        if (readi) std::reverse(readi + r0, readi + r1);
        std::swap(leftclip, rightclip);
    }
    info[DM_MAP_LEFTCLIP] = leftclip;
    info[DM_MAP_RIGHTCLIP] = rightclip;
    // ---- CpG special alignment (:684-704), in place, ascending, later rows see earlier swaps ----
    // (cpg_swap false: getfeatures with a motif other than CG or with position lists, myGetFeatureBasedPos.py:302 - xyrows.inc)
    for (int64_t a = 0; cpg_swap && a < n_rows; ++a) {
        // (both cases need a gap right next to row a: one byte compare per row decides for nearly all of them)
        if (!((a + 1 < n_rows && qb[a + 1] == '-') || (a > 0 && qb[a - 1] == '-'))) continue;
        if (tb[a] == 'C' && qb[a] == 'C') {
            if (a + 1 < n_rows && qb[a + 1] == '-' && tb[a + 1] == 'G') {
                int64_t add = 2;
                while (a + add < n_rows && qb[a + add] == '-' && tb[a + add] == 'G') ++add;
                if (a + add < n_rows && qb[a + add] == 'G' && tb[a + add] == 'G') std::swap(qb[a + 1], qb[a + add]);
            }
        }
        if (tb[a] == 'G' && qb[a] == 'G') {
            if (a - 1 > -1 && qb[a - 1] == '-' && tb[a - 1] == 'C') {
                int64_t add = 2;
                while (a - add > -1 && qb[a - add] == '-' && tb[a - add] == 'C') ++add;
                if (a - add > -1 && qb[a - add] == 'C' && tb[a - add] == 'C') std::swap(qb[a - 1], qb[a - add]);
            }
        }
    }
    info[DM_MAP_STATUS] = DM_MAP_OK;
    return DM_OK;
}

}  // namespace readmap

extern "C" {

int dm_map_read(int flag, int64_t pos1, const char* cigar, const char* readseq, int64_t readseq_len,
                const char* refseq, int64_t refseq_len, int64_t n_events, char* refbase, char* readbase,
                uint64_t* refbasei, uint64_t* readbasei, int64_t cap_rows, int64_t* info) {
    if (!cigar || !readseq || !refseq || !info) return fail(DM_EINVAL, "dm_map_read: null argument");
    // the untrimmed table lives in scratch columns of this thread; the caller gets the final rows if they fit
    thread_local std::vector<char> s_refb, s_readb;
    thread_local std::vector<int64_t> s_refi;
    thread_local std::vector<uint64_t> s_readi;
    int64_t first = 0, need = 0;
    int rc = readmap::map_read_core(flag, pos1, cigar, readseq, readseq_len, refseq, refseq_len, n_events, s_refb.data(), s_readb.data(), s_refi.data(),
                                    s_readi.data(), int64_t(std::min(std::min(s_refb.size(), s_readb.size()), std::min(s_refi.size(), s_readi.size()))), info, &first, &need);
    if (rc == DM_OK && info[DM_MAP_STATUS] == DM_MAP_NEED_ROWS) {
        const size_t want = size_t(need) + (size_t(need) >> 2) + 64;
        s_refb.resize(want);
        s_readb.resize(want);
        s_refi.resize(want);
        s_readi.resize(want);
        rc = readmap::map_read_core(flag, pos1, cigar, readseq, readseq_len, refseq, refseq_len, n_events, s_refb.data(), s_readb.data(), s_refi.data(),
                                    s_readi.data(), int64_t(want), info, &first, &need);
    }
    if (rc != DM_OK || info[DM_MAP_STATUS] != DM_MAP_OK) return rc;
    const int64_t n_rows = info[DM_MAP_N_ROWS];
    if (n_rows > cap_rows || !refbase || !readbase || !refbasei || !readbasei) {
        info[DM_MAP_STATUS] = DM_MAP_NEED_ROWS;    // call again with cap_rows >= info[DM_MAP_N_ROWS]
        return DM_OK;
    }
    std::memcpy(refbase, s_refb.data() + first, size_t(n_rows));
    std::memcpy(readbase, s_readb.data() + first, size_t(n_rows));
    std::memcpy(refbasei, s_refi.data() + first, size_t(n_rows) * 8);
    std::memcpy(readbasei, s_readi.data() + first, size_t(n_rows) * 8);
    return DM_OK;
}

}  // extern "C"
