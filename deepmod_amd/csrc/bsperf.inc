// bsperf.inc — `bsperf`, the line routine (plain C++: part of offline.hip through bsperf.hip.inc, and compiled by g++ as it stands:
// tests/bsperf_asan_driver.cpp).  One line of a bisulfite bedMethyl replicate -> its class and, for a kept line, its record.  The kernel of
// bsperf.hip.inc and dm_bsperf_parse_host run this one routine, so the device and the host cannot disagree on a line.
//
// The reading rules are readBed's (hm_cluster_predict.py:20-41; cluster_train.read_truth): the first line of a FILE is skipped unread (the
// caller says which chunk starts a file); a line whose length without leading and trailing ' ' / '\t' is <= 20 is skipped; a kept line has
// exactly 11 fields, of which 0 (contig), 1 (position), 5 (strand), 9 (coverage) and 10 (percentage) are used; a line with coverage 0 is dropped.
// Grammar of a kept line (parse_line, on the routines of bedline.inc; the '\n' is not part of it): fields of printable bytes (0x21 - 0x7e) separated by runs of one or more
// ' ' / '\t', leading and trailing runs allowed; exactly 11 fields; fields 1, 9, 10 are 1 - 10 digits with a value <= 2^31 - 1; field 10 is
// <= 100; the position of a line of a requested contig is below that contig's limit (its length, or 2^31 - 1).  Outside are 10 or 12 fields,
// '\r', a sign, 11 digits, a percentage of 101, a position beyond the contig.
// Classes, decided in this order on a line inside the grammar: strand neither '+' nor '-' (skipped and counted), contig not among the requested
// names (compared byte for byte: chr1 is neither chr10 nor chr), coverage 0 (dropped), record.
#pragma once
#include "bedline.inc"

#define BS_HD BED_HD

namespace bsk {

constexpr int MAX_CONTIGS = 64;
constexpr int MAX_NAME = 63;
constexpr int MAX_THR = 8;
constexpr int MAX_REP = 4;
constexpr int NPCT = 101;
constexpr long long MAX_LENGTH = 0x7fffffffLL;      // positions 0 .. 2^31 - 2
constexpr int MAX_COV = 65535;                      // a record's coverage saturates here
constexpr int SHORT_LINE = 20;

struct Names {
    char s[MAX_CONTIGS][MAX_NAME + 1];
    int len[MAX_CONTIGS];
    long long limit[MAX_CONTIGS];                   // positions of the contig (a position at or beyond it is outside the grammar)
    int n;
};

enum { L_RECORD, L_HEADER, L_SHORT, L_STRAND, L_CONTIG, L_ZERO, N_LINE };
constexpr int L_BAD = -1;

// a record: the position, and meta = coverage (16 bits, saturated) | percentage << 16 | strand << 23 | contig index << 24
struct Rec {
    int pos;
    unsigned meta;
};

BS_HD inline unsigned pack_meta(const int contig, const int strand, const long long cov, const int pct) {
    return unsigned(cov > MAX_COV ? MAX_COV : cov) | (unsigned(pct) << 16) | (unsigned(strand) << 23) | (unsigned(contig) << 24);
}
BS_HD inline int meta_cov(const unsigned m) { return int(m & 0xffffu); }
BS_HD inline int meta_pct(const unsigned m) { return int((m >> 16) & 0x7fu); }
BS_HD inline int meta_strand(const unsigned m) { return int((m >> 23) & 1u); }
BS_HD inline int meta_contig(const unsigned m) { return int(m >> 24); }

// One line p[0 .. n) (without its '\n') -> its class (L_RECORD: r is its record; L_BAD: outside the grammar).  Reads p[0 .. n) only.
BS_HD inline int parse_line(const char* p, const long long n, const Names& names, Rec& r) {
    long long i = 0, hi = n;
    bed::skip_seps(p, n, i);
    while (hi > i && bed::is_sep(p[hi - 1])) --hi;
    if (hi - i <= SHORT_LINE) return L_SHORT;
    long long b, len, name_b = 0, name_len = 0, strand_b = 0, strand_len = 0;
    long long num[3] = {0, 0, 0};                   // fields 1, 9, 10
    int f = 0;
    for (; i < hi; bed::skip_seps(p, hi, i)) {
        if (bed::next_field(p, hi, i, b, len) != bed::F_FIELD) return L_BAD;
        if (f == 0) {
            name_b = b;
            name_len = len;
        } else if (f == 1 || f == 9 || f == 10) {
            if (!bed::parse_u31(p, b, i, num[f == 1 ? 0 : f - 8])) return L_BAD;
        } else if (f == 5) {
            strand_b = b;
            strand_len = len;
        }
        if (++f > 11) return L_BAD;
    }
    if (f != 11 || num[2] > 100) return L_BAD;
    unsigned char strand;
    if (!bed::strand_of(p, strand_b, strand_len, strand)) return L_STRAND;
    int c = -1;
    for (int k = 0; k < names.n && c < 0; ++k)
        if (bed::same_bytes(p, name_b, name_len, names.s[k], names.len[k])) c = k;
    if (c < 0) return L_CONTIG;
    if (num[0] >= names.limit[c]) return L_BAD;
    if (num[1] == 0) return L_ZERO;
    r.pos = int(num[0]);
    r.meta = pack_meta(c, strand, num[1], int(num[2]));
    return L_RECORD;
}

// 1 to MAX_CONTIGS distinct names of 1 to MAX_NAME printable bytes; lengths: null or < 0: none given.  -> 0, or 1 + the index of the name refused
inline int set_names(Names& names, const int n, const char* const* list, const int64_t* lengths) {
    std::memset(&names, 0, sizeof names);
    if (n < 1 || n > MAX_CONTIGS || !list) return 1;
    for (int k = 0; k < n; ++k) {
        const size_t len = list[k] ? std::strlen(list[k]) : 0;
        if (len < 1 || len > size_t(MAX_NAME) || !bed::printable(list[k], (long long)len)) return k + 1;
        for (int q = 0; q < k; ++q)
            if (size_t(names.len[q]) == len && std::memcmp(names.s[q], list[k], len) == 0) return k + 1;
        std::memcpy(names.s[k], list[k], len);
        names.len[k] = int(len);
        const int64_t given = lengths ? lengths[k] : -1;
        if (given == 0 || given > MAX_LENGTH) return k + 1;
        names.limit[k] = given < 0 ? MAX_LENGTH : given;
    }
    names.n = n;
    return 0;
}

// The text [0, n_bytes) line by line (a last line without '\n' ends with the text) -> its records in line order, as many as fit `cap`;
// -> records.  lines [N_LINE]: the lines of every class; *bad: the first line outside the grammar (1-based), 0: none.
inline int64_t parse_text(const char* text, const int64_t n_bytes, const Names& names, const bool first_chunk, int32_t* pos, uint32_t* meta, const int64_t cap,
                          int64_t* lines, int64_t* bad) {
    int64_t recs = 0;
    for (int k = 0; k < N_LINE; ++k) lines[k] = 0;
    bed::for_each_line(text, n_bytes, bad, [&](const char* line, const int64_t len, const int64_t row) {
        Rec v = {0, 0};
        const int cls = (first_chunk && row == 0) ? int(L_HEADER) : parse_line(line, len, names, v);
        if (cls == L_BAD) return false;
        ++lines[cls];
        if (cls == L_RECORD) {
            if (recs < cap) {
                pos[recs] = v.pos;
                meta[recs] = v.meta;
            }
            ++recs;
        }
        return true;
    });
    return recs;
}

}  // namespace bsk
