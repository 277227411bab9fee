// xyrows.inc — getfeatures, host part (host C++, part of offline.hip): alignment table + position lists -> labelled matrix rows, and the
// definition of the .xy.gz text.
//
// Replaces, of the reference's bin/DeepMod_scripts/myGetFeatureBasedPos.py:
//   :135-138  a read on a contig without a listed position is skipped                                   DM_XY_NO_SITE
//   :146-319  handle_record's alignment walk = myDetect's (readmap.inc), the CpG gap swap only with motif 'CG' (:302)
//   :321-323  fewer than 500 aligned events                                                               DM_XY_LESS_EVENT
//   :377-444  get_Feature's cgpos walk: positive positions (cgpos[0]) and excluded positions (cgpos[1])
//   :448-492  reference position and the negative / positive label of every aligned event
//   :512-526  the +-25 row selection, and np.savetxt(fmt='%.3f') of the kept rows (dm_xy_rows_host: what xyrows.hip.inc computes on the device)
// A matrix row is (pos, lab, code) here: pos = column 0, lab = 0 none | 1 negative (column 1) | 2 positive (column 2), code = the one-hot class
// dm_rows_assemble takes (0..3 = A C G T, 255 none); columns 7..9 are the (mean, stdv, length) of the event the row shows (rdesc, as dm_rows_assemble).
// Membership is by (strand, refbasei) VALUE as in the reference: the lists are sorted arrays per contig x strand, cgpos two sorted arrays per read.
#pragma once
#include "host.h"

struct dm_xysites {
    int32_t n_contigs = 0;
    bool has_any = false, has_no = false;              // anymodlist / nomodlist are not None (--motifORPos 2)
    std::vector<std::vector<int64_t>> list;            // [(contig * 2 + strand) * 3 + kind], sorted, unique
    const std::vector<int64_t>& of(int32_t contig, int strand, int kind) const { return list[(size_t(contig) * 2 + size_t(strand)) * 3 + size_t(kind)]; }
    bool contig_listed(int32_t contig) const {
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 3; ++k)
                if ((k == 0 || (k == 1 && has_any) || (k == 2 && has_no)) && !of(contig, s, k).empty()) return true;
        return false;
    }
};

namespace xyhost {

inline bool in_sorted(const std::vector<int64_t>& v, int64_t p) { return std::binary_search(v.begin(), v.end(), p); }

inline uint8_t onehot_code(char b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 255; }

// :377-444.  c0 / c1 = cgpos[0] / cgpos[1] as sorted unique reference positions (the strand of every entry is the read's)
inline void cgpos_walk(const std::vector<int64_t>& ful, const char* motif, int motif_pos, const char* refb, const char* readb, const int64_t* refi, int64_t n,
                       std::vector<int64_t>& c0, std::vector<int64_t>& c1) {
    c0.clear();
    c1.clear();
    const int64_t L = motif ? int64_t(std::strlen(motif)) : 0;
    for (int64_t a = 0; a < n; ++a) {
        // the motif in the read but not in the reference (:379-382): the base and its neighbours are not used
        if (motif && readb[a] == motif[motif_pos]) {
            const int64_t st = a - motif_pos, en = a + L - motif_pos;
            if (st > -1 && en <= n && std::memcmp(readb + st, motif, size_t(L)) == 0 && std::memcmp(refb + st, motif, size_t(L)) != 0)
                for (int64_t addi = std::max<int64_t>(a - 1, 0); addi < std::min<int64_t>(a + 2, n); ++addi) c1.push_back(refi[addi]);
        }
        if (refb[a] == '-' || readb[a] == '-' || !in_sorted(ful, refi[a])) continue;
        int64_t nextnogap = a + 1;
        while (nextnogap < n && refb[nextnogap] == '-') ++nextnogap;
        bool iscg = false;
        for (int cn = 3; cn <= 6 && !iscg && nextnogap < n; cn += 3) {           // the gap test over +-3 and +-6 table rows (:392-406)
            int gapnum = 0;
            for (int64_t c = a - cn; c <= a + cn; ++c)
                if (c > -1 && c < n && (refb[c] == '-' || readb[c] == '-')) ++gapnum;
            if (gapnum <= (cn == 3 ? 2 : 3)) {
                for (int64_t addi = std::max<int64_t>(a - 1, 0); addi < std::min<int64_t>(nextnogap + 1, n); ++addi) (addi == a ? c0 : c1).push_back(refi[addi]);
                iscg = true;
            }
        }
        if (iscg) continue;
        // too many gaps: the site and what lies between its neighbours in the reference and in the read are not used (:409-444)
        nextnogap = a + 1;
        while (nextnogap < n && refb[nextnogap] == '-') ++nextnogap;
        int64_t prenogap = a - 1;
        while (prenogap > -1 && refb[prenogap] == '-') --prenogap;
        int64_t read0 = a - 1, read1 = a + 1;
        while (read0 > -1 && readb[read0] == '-') --read0;
        while (read1 < n && readb[read1] == '-') ++read1;
        if (read0 < prenogap) prenogap = read0 > -1 ? read0 : 0;
        if (read1 > nextnogap) nextnogap = read1 < n ? read1 : n - 1;
        if (prenogap < 0) prenogap = 0;
        if (!(nextnogap < n)) nextnogap = n - 1;
        if (!(prenogap < n)) prenogap = n - 1;
        for (int64_t e = prenogap; e <= nextnogap; ++e) c1.push_back(refi[e]);
    }
    for (std::vector<int64_t>* c : {&c0, &c1}) {
        std::sort(c->begin(), c->end());
        c->erase(std::unique(c->begin(), c->end()), c->end());
    }
}

// get_Feature's rows of one read (:365-369, :448-492) -> the matrix rows, or a DM_XY_* status with nothing promised about the arrays
inline int label_rows(const dm_xysites* s, int32_t contig, int strand, const char* motif, int motif_pos, int posneg, const char* refb, const char* readb,
                      const int64_t* refi, int64_t n, int64_t n_events, int64_t start_clip, int64_t end_clip, int64_t mapped_start_pos,
                      int64_t num_insertions, int64_t* pos, uint8_t* lab, uint8_t* code, int64_t cap_rows, int64_t* n_rows) {
    const int64_t n_al = n_events - end_clip - start_clip;          // aligned events; the matrix has 100 rows more on either side
    *n_rows = n_al + 200;
    if (n_al < 0 || start_clip < 0 || end_clip < 0) return DM_XY_INDEX_ERROR;
    if (*n_rows > cap_rows) return DM_XY_NEED_ROWS;
    const std::vector<int64_t>& ful = s->of(contig, strand, 0);
    const std::vector<int64_t>& any = s->of(contig, strand, 1);
    const std::vector<int64_t>& no = s->of(contig, strand, 2);
    thread_local std::vector<int64_t> tl_c0, tl_c1;
    std::vector<int64_t>&c0 = tl_c0, &c1 = tl_c1;
    if (posneg != 0) cgpos_walk(ful, motif, motif_pos, refb, readb, refi, n, c0, c1);
    std::memset(pos, 0, size_t(*n_rows) * sizeof(int64_t));
    std::memset(lab, 0, size_t(*n_rows));
    std::memset(code, 255, size_t(*n_rows));
    const int64_t step = strand == 0 ? 1 : -1;
    int64_t align_ref_pos = strand == 0 ? mapped_start_pos : mapped_start_pos + n - num_insertions - 1;
    int64_t a = 0;
    for (int64_t k = 0; k < n_al; ++k) {
        while (a < n && readb[a] == '-') {
            if (refb[a] != '-') align_ref_pos += step;
            ++a;
        }
        if (a >= n) return DM_XY_INDEX_ERROR;                       // the reference raises IndexError (:455)
        const int64_t row = 100 + k, key = refi[a];
        pos[row] = align_ref_pos;
        code[row] = onehot_code(refb[a]);
        if (posneg == 0) {                                          // :469-475
            if ((s->has_any && s->has_no && in_sorted(no, key)) || in_sorted(ful, key) || (s->has_any && in_sorted(any, key))) lab[row] = 1;
        } else if (refb[a] != '-' && in_sorted(c0, key)) {          // :477-478
            lab[row] = 2;
        } else if (!in_sorted(c1, key)) {                           // :480-488
            if (!(s->has_any && in_sorted(any, key)) && (!s->has_no || in_sorted(no, key))) lab[row] = 1;
        }
        if (refb[a] != '-') align_ref_pos += step;
        ++a;
    }
    return DM_XY_OK;
}

inline void set_rdesc(int64_t* rdesc, int64_t row0, int64_t ev0, int64_t n_events, int64_t start_clip) {
    if (!rdesc) return;
    rdesc[0] = row0;                                    // row q of the batch shows event q + rdesc[1] if that lies in [rdesc[2], rdesc[3])
    rdesc[1] = ev0 + start_clip - 100 - row0;
    rdesc[2] = ev0;
    rdesc[3] = ev0 + n_events;
}

// '%.3f' % v as Python prints it (np.savetxt): the correctly rounded decimal, 'nan' without a sign, 'inf' / '-inf'
inline int format_value(char* out, size_t cap, double v) {
    if (std::isnan(v)) return std::snprintf(out, cap, "nan");
    return std::snprintf(out, cap, "%.3f", v);
}

// the descriptors of a batch, checked before anything is indexed with them: rows of read r = [rdesc[4 r], rdesc[4 (r + 1)]) (the last read ends at
// n_rows), not empty, in order; the events a row can show lie in the block of n_events events
inline int check_rdesc(const int64_t* rdesc, int64_t n_reads, int64_t n_rows, int64_t n_events, const char* who) {
    if (n_reads <= 0 || n_reads > 0x7fffffffLL || n_rows <= 0 || n_events < 0 || !rdesc) return fail(DM_EINVAL, "%s: no read, no row or a null table", who);
    if (n_rows > (int64_t(1) << 40) || n_events > (int64_t(1) << 40)) return fail(DM_EINVAL, "%s: more than 2^40 rows or events", who);
    if (rdesc[0] != 0) return fail(DM_EINVAL, "%s: the first read does not start at row 0", who);
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t* d = rdesc + 4 * r;
        const int64_t end = r + 1 < n_reads ? d[4] : n_rows;
        if (d[0] < 0 || end <= d[0] || end > n_rows) return fail(DM_EINVAL, "%s: read %lld covers rows %lld .. %lld of %lld", who, (long long)r, (long long)d[0], (long long)end, (long long)n_rows);
        if (d[2] < 0 || d[3] < d[2] || d[3] > n_events) return fail(DM_EINVAL, "%s: read %lld shows events %lld .. %lld of %lld", who, (long long)r, (long long)d[2], (long long)d[3], (long long)n_events);
        if (d[1] < -(int64_t(1) << 41) || d[1] > (int64_t(1) << 41)) return fail(DM_EINVAL, "%s: read %lld: row to event shift %lld", who, (long long)r, (long long)d[1]);
    }
    return DM_OK;
}

}  // namespace xyhost

extern "C" {

dm_xysites* dm_xy_sites_create(int32_t n_contigs, int has_any, int has_no) {
    if (n_contigs <= 0 || n_contigs > (1 << 24)) {
        fail(DM_EINVAL, "dm_xy_sites_create: %d contigs", n_contigs);
        return nullptr;
    }
    dm_xysites* s = new dm_xysites;
    s->n_contigs = n_contigs;
    s->has_any = has_any != 0;
    s->has_no = has_no != 0;
    s->list.resize(size_t(n_contigs) * 6);
    return s;
}

void dm_xy_sites_destroy(dm_xysites* s) { delete s; }

// kind: 0 fulmodlist, 1 anymodlist, 2 nomodlist.  The positions are copied, sorted and made unique.
int dm_xy_sites_set(dm_xysites* s, int32_t contig, int strand, int kind, const int64_t* pos, int64_t n) {
    if (!s || contig < 0 || contig >= s->n_contigs || (strand != 0 && strand != 1) || kind < 0 || kind > 2 || n < 0 || (n > 0 && !pos))
        return fail(DM_EINVAL, "dm_xy_sites_set: contig %d strand %d kind %d n %lld", contig, strand, kind, (long long)n);
    std::vector<int64_t>& v = s->list[(size_t(contig) * 2 + size_t(strand)) * 3 + size_t(kind)];
    v.assign(pos, pos + n);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return DM_OK;
}

int dm_xy_labels(const dm_xysites* s, int32_t contig, int strand, const char* motif, int motif_pos, int posneg, const char* refbase, const char* readbase,
                 const uint64_t* refbasei, int64_t n_table_rows, int64_t n_events, int64_t start_clip, int64_t end_clip, int64_t mapped_start_pos,
                 int64_t num_insertions, int64_t* pos, uint8_t* lab, uint8_t* code, int64_t cap_rows, int64_t row0, int64_t ev0, int64_t* rdesc,
                 int64_t* info) {
    if (!s || !refbase || !readbase || !refbasei || !info || n_table_rows < 0 || n_events < 0) return fail(DM_EINVAL, "dm_xy_labels: null argument");
    if (contig < 0 || contig >= s->n_contigs || (strand != 0 && strand != 1)) return fail(DM_EINVAL, "dm_xy_labels: contig %d, strand %d", contig, strand);
    if (motif && (motif_pos < 0 || size_t(motif_pos) >= std::strlen(motif))) return fail(DM_EINVAL, "dm_xy_labels: position %d in motif '%s'", motif_pos, motif);
    if (cap_rows > 0 && (!pos || !lab || !code)) return fail(DM_EINVAL, "dm_xy_labels: null output");
    for (int i = 0; i < DM_XY_INFO_LEN; ++i) info[i] = 0;
    info[DM_XY_STRAND] = strand;
    info[DM_XY_START_CLIP] = start_clip;
    info[DM_XY_END_CLIP] = end_clip;
    int64_t n_rows = 0;
    info[DM_XY_STATUS] = xyhost::label_rows(s, contig, strand, motif, motif_pos, posneg, refbase, readbase, reinterpret_cast<const int64_t*>(refbasei),
                                            n_table_rows, n_events, start_clip, end_clip, mapped_start_pos, num_insertions, pos, lab, code, cap_rows, &n_rows);
    info[DM_XY_N_ROWS] = n_rows;
    if (info[DM_XY_STATUS] == DM_XY_OK) xyhost::set_rdesc(rdesc, row0, ev0, n_events, start_clip);
    return DM_OK;
}

int dm_xy_read(const dm_xysites* s, int32_t contig, int flag, int64_t pos1, const char* cigar, const char* readseq, int64_t readseq_len, const char* refseq,
               int64_t refseq_len, int64_t n_events, const char* motif, int motif_pos, int posneg, int64_t* pos, uint8_t* lab, uint8_t* code,
               int64_t cap_rows, int64_t row0, int64_t ev0, int64_t* rdesc, int64_t* info) {
    if (!s || !cigar || !readseq || !refseq || !info || n_events < 0) return fail(DM_EINVAL, "dm_xy_read: null argument");
    if (contig < 0 || contig >= s->n_contigs) return fail(DM_EINVAL, "dm_xy_read: contig %d", contig);
    if (motif && (motif_pos < 0 || size_t(motif_pos) >= std::strlen(motif))) return fail(DM_EINVAL, "dm_xy_read: position %d in motif '%s'", motif_pos, motif);
    if (cap_rows > 0 && (!pos || !lab || !code)) return fail(DM_EINVAL, "dm_xy_read: null output");
    for (int i = 0; i < DM_XY_INFO_LEN; ++i) info[i] = 0;
    if (!s->contig_listed(contig)) {                                // :135-138
        info[DM_XY_STATUS] = DM_XY_NO_SITE;
        return DM_OK;
    }
    thread_local std::vector<char> s_refb, s_readb;
    thread_local std::vector<int64_t> s_refi;
    const bool cpg_swap = motif && std::strcmp(motif, "CG") == 0;   // :302
    int64_t minfo[DM_MAP_INFO_LEN], first = 0, need = 0;
    int rc = readmap::map_read_core(flag, pos1, cigar, readseq, readseq_len, refseq, refseq_len, n_events, s_refb.data(), s_readb.data(), s_refi.data(), nullptr,
                                    int64_t(std::min(s_refb.size(), std::min(s_readb.size(), s_refi.size()))), minfo, &first, &need, cpg_swap);
    if (rc == DM_OK && minfo[DM_MAP_STATUS] == DM_MAP_NEED_ROWS) {
        const size_t want = size_t(need) + (size_t(need) >> 2) + 64;
        s_refb.resize(want);
        s_readb.resize(want);
        s_refi.resize(want);
        rc = readmap::map_read_core(flag, pos1, cigar, readseq, readseq_len, refseq, refseq_len, n_events, s_refb.data(), s_readb.data(), s_refi.data(), nullptr,
                                    int64_t(want), minfo, &first, &need, cpg_swap);
    }
    if (rc != DM_OK) return rc;
    info[DM_XY_STRAND] = minfo[DM_MAP_STRAND];
    info[DM_XY_POS_AFTER_CLIP] = minfo[DM_MAP_POS_AFTER_CLIP];
    info[DM_XY_EVENTS_AFTER_CLIP] = minfo[DM_MAP_EVENTS_AFTER_CLIP];
    if (minfo[DM_MAP_STATUS] != DM_MAP_OK) {
        info[DM_XY_STATUS] = DM_XY_NO_MATCH;                        // :245-250
        return DM_OK;
    }
    info[DM_XY_START_CLIP] = minfo[DM_MAP_LEFTCLIP];
    info[DM_XY_END_CLIP] = minfo[DM_MAP_RIGHTCLIP];
    if (minfo[DM_MAP_EV_HI] - minfo[DM_MAP_EV_LO] < 500) {          // :321-323
        info[DM_XY_STATUS] = DM_XY_LESS_EVENT;
        return DM_OK;
    }
    int64_t n_rows = 0;
    info[DM_XY_STATUS] = xyhost::label_rows(s, contig, int(minfo[DM_MAP_STRAND]), motif, motif_pos, posneg, s_refb.data() + first, s_readb.data() + first,
                                            s_refi.data() + first, minfo[DM_MAP_N_ROWS], n_events, minfo[DM_MAP_LEFTCLIP], minfo[DM_MAP_RIGHTCLIP],
                                            minfo[DM_MAP_FIRST_MATCH_POS], minfo[DM_MAP_NUM_INSERT], pos, lab, code, cap_rows, &n_rows);
    info[DM_XY_N_ROWS] = n_rows;
    if (info[DM_XY_STATUS] == DM_XY_OK) xyhost::set_rdesc(rdesc, row0, ev0, n_events, minfo[DM_MAP_LEFTCLIP]);
    return DM_OK;
}

int64_t dm_xy_format_host(const double* rows, int64_t n_rows, char* out, int64_t cap) {
    if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(DM_EINVAL, "dm_xy_format_host: null rows");
    int64_t total = 0;
    char buf[512];                                                  // '%.3f' of a double has at most 309 + 5 characters
    for (int pass = 0; pass < 2; ++pass) {
        char* w = out;
        for (int64_t r = 0; r < n_rows; ++r)
            for (int c = 0; c < 10; ++c) {
                const int k = xyhost::format_value(buf, sizeof buf, rows[10 * r + c]);
                if (pass == 0) {
                    total += k + 1;
                } else {
                    std::memcpy(w, buf, size_t(k));
                    w[k] = c == 9 ? '\n' : ' ';
                    w += k + 1;
                }
            }
        if (pass == 0 && (!out || cap < total)) break;              // sized first: nothing is written into a buffer that is too small
    }
    return total;
}

// The device stage of a batch (xyrows.hip.inc) on the host, from downloaded statistics: selection (:512-526), then the text of the kept rows.  This is
// what dm_xy_rows returns for a batch whose values the device formatter does not take (NaN, Inf, 2^30 and beyond).  keep [n_rows], read_row_off,
// read_byte_off [n_reads + 1] and text are optional; -> the bytes of the text.
int64_t dm_xy_rows_host(const int64_t* pos, const uint8_t* lab, const uint8_t* code, const int64_t* rdesc, int64_t n_reads, int64_t n_rows, const float* ev3,
                        int64_t n_events, uint8_t* keep, int64_t* read_row_off, int64_t* read_byte_off, char* text, int64_t cap) {
    if (!pos || !lab || !code || (n_events > 0 && !ev3)) return fail(DM_EINVAL, "dm_xy_rows_host: null array");
    const int rc = xyhost::check_rdesc(rdesc, n_reads, n_rows, n_events, "dm_xy_rows_host");
    if (rc) return rc;
    std::vector<uint8_t> kp(size_t(n_rows), 0);
    int64_t out_row = 0, out_byte = 0;
    double row[10];
    char buf[512];
    for (int64_t r = 0; r < n_reads; ++r) {
        const int64_t* d = rdesc + 4 * r;
        const int64_t r0 = d[0], r1 = r + 1 < n_reads ? d[4] : n_rows, n = r1 - r0;
        int64_t kept = 0, next_free = r0;                           // rows below next_free are decided
        for (int64_t q = r0; q < r1; ++q)
            if (lab[q]) {
                const int64_t hi = std::min(q + 25, r1 - 1);
                for (int64_t j = std::max(next_free, std::max(q - 25, r0)); j <= hi; ++j) {
                    kp[size_t(j)] = 1;
                    ++kept;
                }
                next_free = std::max(next_free, hi + 1);
            }
        if (kept > 0 && 10 * kept > 9 * n) {                        // len(keepInd) > len(mfeatures) * 0.9: the whole matrix
            std::memset(kp.data() + r0, 1, size_t(n));
            kept = n;
        }
        if (read_row_off) read_row_off[r] = out_row;
        if (read_byte_off) read_byte_off[r] = out_byte;
        out_row += kept;
        for (int64_t q = r0; q < r1 && kept > 0; ++q) {
            if (!kp[size_t(q)]) continue;
            const int64_t e = q + d[1];
            const bool has = e >= d[2] && e < d[3];
            row[0] = double(pos[q]);
            row[1] = lab[q] == 1 ? 1.0 : 0.0;
            row[2] = lab[q] == 2 ? 1.0 : 0.0;
            for (int c = 0; c < 4; ++c) row[3 + c] = code[q] == c ? 1.0 : 0.0;
            for (int c = 0; c < 3; ++c) row[7 + c] = has ? double(ev3[3 * e + c]) : 0.0;
            for (int c = 0; c < 10; ++c) {
                const int k = xyhost::format_value(buf, sizeof buf, row[c]);
                if (text && out_byte + k + 1 <= cap) {
                    std::memcpy(text + out_byte, buf, size_t(k));
                    text[out_byte + k] = c == 9 ? '\n' : ' ';
                }
                out_byte += k + 1;
            }
        }
    }
    if (read_row_off) read_row_off[n_reads] = out_row;
    if (read_byte_off) read_byte_off[n_reads] = out_byte;
    if (keep) std::memcpy(keep, kp.data(), size_t(n_rows));
    return out_byte;
}

}  // extern "C"
