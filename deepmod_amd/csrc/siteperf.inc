// siteperf.inc — `siteperf`, the line routine (plain C++: part of offline.hip through siteperf.hip.inc, and compiled by g++ as it stands:
// tests/siteperf_asan_driver.cpp).  One BED line of a run or of a control run -> its record.  sp_parse_kernel of siteperf.hip.inc and
// dm_siteperf_parse_host run this one routine, so the device and the host cannot disagree on a line.
//
// Grammar of a line (parse_line, on the routines of bedline.inc; the '\n' is not part of it): at least 12 fields of printable bytes, exactly one
// ' ' or '\t' between two fields and none at either end; field 0 is the contig's name byte for byte; fields 1, 9, 10, 11 (position, coverage,
// percentage, modified) are 1 - 10 digits with a value <= 2^31 - 1; the position lies on the contig, the percentage is <= 100, the modified
// count is <= the coverage; field 3 (the base) is one byte; field 5 is '+' or '-'.  Outside are '\r', an empty line, two separators in a row,
// another contig, a sign, 11 fields, 11 digits.
#pragma once
#include "bedline.inc"

namespace spk {

struct Rec {
    int pos, cov, pct, mod;
    unsigned char strand, base;                     // strand 0 '+', 1 '-'
};

// One line p[0 .. n) (without its '\n') -> its record; false: outside the grammar (r is then unspecified).  Reads p[0 .. n) only.
BED_HD inline bool parse_line(const char* p, const long long n, const bed::Name& name, const long long contig_len, Rec& r) {
    long long i = 0, b, len;
    long long num[4] = {0, 0, 0, 0};                // fields 1, 9, 10, 11
    int f = 0;
    for (;; ++i) {                                  // over the one separator behind a field
        if (bed::next_field(p, n, i, b, len) != bed::F_FIELD) return false;      // an empty line, two separators in a row, a separator at either end
        if (f == 0) {
            if (!bed::same_bytes(p, b, len, name.s, name.n)) return false;
        } else if (f == 1 || (f >= 9 && f <= 11)) {
            if (!bed::parse_u31(p, b, i, num[f == 1 ? 0 : f - 8])) return false;
        } else if (f == 3) {
            if (len != 1) return false;
            r.base = (unsigned char)p[b];
        } else if (f == 5) {
            if (!bed::strand_of(p, b, len, r.strand)) return false;
        }
        if (f < 12) ++f;
        if (i == n) break;
    }
    if (f < 12) return false;
    if (num[0] >= contig_len || num[2] > 100 || num[3] > num[1]) return false;
    r.pos = int(num[0]);
    r.cov = int(num[1]);
    r.pct = int(num[2]);
    r.mod = int(num[3]);
    return true;
}

// The text [0, n_bytes) line by line -> its records, as many as fit `cap` (a line outside the grammar: zeros); -> lines.
// *bad: the first line outside the grammar (1-based), 0: none.
inline int64_t parse_text(const char* text, const int64_t n_bytes, const bed::Name& name, const long long contig_len, int32_t* pos, uint8_t* strand, uint8_t* base,
                          int32_t* cov, int32_t* pct, int32_t* mod, const int64_t cap, int64_t* bad) {
    return bed::for_each_line(text, n_bytes, bad, [&](const char* line, const int64_t len, const int64_t row) {
        Rec v = {0, 0, 0, 0, 0, 0};
        const bool ok = parse_line(line, len, name, contig_len, v);
        if (row < cap) {
            pos[row] = ok ? v.pos : 0;
            cov[row] = ok ? v.cov : 0;
            pct[row] = ok ? v.pct : 0;
            mod[row] = ok ? v.mod : 0;
            strand[row] = ok ? v.strand : 0;
            base[row] = ok ? v.base : 0;
        }
        return ok;
    });
}

}  // namespace spk
