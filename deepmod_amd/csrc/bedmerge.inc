// bedmerge.inc — `merge`, the line routines (plain C++: part of offline.hip through bedmerge.hip.inc, and compiled by g++ as it stands:
// tests/merge_asan_driver.cpp).  One BED line -> its (position, strand, coverage, modified) record, and one (position, strand) of the summed
// tables -> its line in the dialect of DeepMod_tools/sum_chr_mod.py:63.  The kernels of bedmerge.hip.inc and the host entry points below run
// the same two routines, so the device and the host cannot disagree on a line.
//
// Grammar of a line (parse_line, on the routines of bedline.inc; the '\n' is not part of it): fields of printable bytes (0x21 - 0x7e) separated by runs of one or more ' ' /
// '\t', leading and trailing runs allowed; at least 12 fields; field 0 is the contig's name byte for byte; fields 1, 9, 11 (position,
// coverage, modified) are 1 - 10 digits with a value <= 2^31 - 1; field 5 is '+' or '-'; modified <= coverage; position < limit (the table
// length, at most 2^31 - 1 so that position + 1 is an int32).  Fields 3 and 10 are not looked at: sum_chr_mod.py never reads them.  Inside
// are what detect writes (single spaces, one before the newline), what sum_chr_mod.py writes (two spaces after the strand) and what
// hm_cluster_predict.py writes (13 fields); outside are '\r', a blank line, another contig, a sign, 11 fields, 11 digits.
//
// A line of the output (emit_line): '%s %d %d %s %d %s  %d %d 0,0,0 %d %d %d\n' % (chr, pos, pos + 1, Base, min(cov, 1000), strand, pos,
// pos + 1, cov, pct, mod), written for mod > 0 only, '+' before '-' at one position.  pct = (100 * mod) / cov in 64-bit integers: with
// 0 < mod <= cov < 2^31 the product is below 2^38, exact as a double, and the double quotient truncates to the integer quotient (a quotient
// that is an integer is exact; any other lies at least 1 / cov > 2^-31 from one, far more than an ulp of a number below 101), so it is
// Python's int(mod * 100 / cov).
#pragma once
#include "bedline.inc"
#include "textout.inc"

#define BM_HD BED_HD

namespace bmk {

using bed::Name;
using txo::put_uint;
constexpr long long MAX_LENGTH = 0x7fffffffLL;      // positions 0 .. 2^31 - 2

struct Rec {
    int pos, cov, mod;
    unsigned char strand;                           // 0 '+', 1 '-'
};

// One line p[0 .. n) (without its '\n') -> its record; false: outside the grammar (r is then unspecified).  Reads p[0 .. n) only.
BM_HD inline bool parse_line(const char* p, const long long n, const Name& name, const long long limit, Rec& r) {
    long long i = 0, b, len;
    long long num[3] = {0, 0, 0};                   // fields 1, 9, 11
    int f = 0;
    r.strand = 0;
    for (;;) {
        bed::skip_seps(p, n, i);
        if (i >= n) break;
        if (bed::next_field(p, n, i, b, len) != bed::F_FIELD) return false;
        if (f == 0) {
            if (!bed::same_bytes(p, b, len, name.s, name.n)) return false;
        } else if (f == 1 || f == 9 || f == 11) {
            if (!bed::parse_u31(p, b, i, num[f == 1 ? 0 : (f == 9 ? 1 : 2)])) return false;
        } else if (f == 5) {
            if (!bed::strand_of(p, b, len, r.strand)) return false;
        }
        if (f < 12) ++f;
    }
    if (f < 12) return false;
    if (num[2] > num[1] || num[0] >= limit) return false;
    r.pos = int(num[0]);
    r.cov = int(num[1]);
    r.mod = int(num[2]);
    return true;
}

// The line of (pos, strand) with the sums cov, mod (0 < mod <= cov).  The same routine counts and writes: the two cannot disagree on a length.
template <class Sink>
BM_HD inline void emit_line(Sink& s, const Name& name, const char base, const long long pos, const int strand, const long long cov, const long long mod) {
    for (int j = 0; j < name.n; ++j) s.put(name.s[j]);
    s.put(' ');
    put_uint(s, (unsigned long long)pos);
    s.put(' ');
    put_uint(s, (unsigned long long)(pos + 1));
    s.put(' ');
    s.put(base);
    s.put(' ');
    put_uint(s, (unsigned long long)(cov < 1000 ? cov : 1000));
    s.put(' ');
    s.put(strand ? '-' : '+');
    s.put(' ');
    s.put(' ');
    put_uint(s, (unsigned long long)pos);
    s.put(' ');
    put_uint(s, (unsigned long long)(pos + 1));
    s.put(' ');
    s.put('0');
    s.put(',');
    s.put('0');
    s.put(',');
    s.put('0');
    s.put(' ');
    put_uint(s, (unsigned long long)cov);
    s.put(' ');
    put_uint(s, (unsigned long long)(cov > 0 ? (100 * mod) / cov : 0));
    s.put(' ');
    put_uint(s, (unsigned long long)mod);
    s.put('\n');
}

// what a sum has to be for the formatter (and for an exact percentage); the overflow guard of the adds keeps the sums here
BM_HD inline bool sum_ok(const long long cov, const long long mod) { return cov >= 0 && mod >= 0 && mod <= cov; }

// The lines of table position q (index i of the arrays; a null strand holds nothing): '+' first.  -> lines emitted
template <class Sink>
BM_HD inline int emit_position(Sink& s, const Name& name, const char base, const long long q, const long long i, const int32_t* cov_p, const int32_t* mod_p,
                               const int32_t* cov_m, const int32_t* mod_m) {
    int lines = 0;
    if (mod_p && mod_p[i] > 0) {
        emit_line(s, name, base, q, 0, cov_p[i], mod_p[i]);
        ++lines;
    }
    if (mod_m && mod_m[i] > 0) {
        emit_line(s, name, base, q, 1, cov_m[i], mod_m[i]);
        ++lines;
    }
    return lines;
}

// The lines of `merge` as an emitter (textout.inc): the four tables, a null strand holds nothing.  The text is defined for sums that are ok; the
// tile writer (textout.hip.inc) skips a position whose sums are not and counts its tile into *bad_tiles (device memory; null on the host, whose
// format_tables looks at the sums before it formats).
struct Emitter {
    Name name;
    char base;
    const int32_t *cov_p, *mod_p, *cov_m, *mod_m;
    unsigned long long* bad_tiles;
    static constexpr bool CHECKED = true;
    BM_HD bool ok(const long long i) const { return (!mod_p || sum_ok(cov_p[i], mod_p[i])) && (!mod_m || sum_ok(cov_m[i], mod_m[i])); }
    template <class Sink>
    BM_HD int operator()(Sink& s, const long long q, const long long i) const {
        return emit_position(s, name, base, q, i, cov_p, mod_p, cov_m, mod_m);
    }
};

// a contig name for `merge`: 1 to bed::MAX_NAME bytes, all of them printable (the name is written into every line of the output)
inline bool set_name(Name& name, const char* contig_name) { return bed::set_name(name, contig_name) && bed::printable(name.s, name.n); }

// The text [0, n_bytes) line by line -> its records, as many as fit `cap` (a line outside the grammar: zeros); -> lines.
// *bad: the first line outside the grammar (1-based), 0: none.
inline int64_t parse_text(const char* text, const int64_t n_bytes, const Name& name, const long long limit, int32_t* pos, uint8_t* strand, int32_t* cov, int32_t* mod,
                          const int64_t cap, int64_t* bad) {
    return bed::for_each_line(text, n_bytes, bad, [&](const char* line, const int64_t len, const int64_t row) {
        Rec v = {0, 0, 0, 0};
        const bool ok = parse_line(line, len, name, limit, v);
        if (row < cap) {
            pos[row] = ok ? v.pos : 0;
            cov[row] = ok ? v.cov : 0;
            mod[row] = ok ? v.mod : 0;
            strand[row] = ok ? v.strand : 0;
        }
        return ok;
    });
}

// The text of positions first_pos .. first_pos + length - 1 from the four tables: counted first; written only if it fits `cap`.
// -> bytes of the text, -1: a sum outside 0 <= mod <= cov (*bad_index: its index).
inline int64_t format_tables(const Name& name, const char base, const int64_t first_pos, const int64_t length, const int32_t* cov_p, const int32_t* mod_p,
                             const int32_t* cov_m, const int32_t* mod_m, char* out, const int64_t cap, int64_t* lines, int64_t* bad_index) {
    const Emitter em = {name, base, cov_p, mod_p, cov_m, mod_m, nullptr};
    for (int64_t i = 0; i < length; ++i)
        if (!em.ok(i)) {
            *bad_index = i;
            return -1;
        }
    return txo::format_range(em, first_pos, length, out, cap, lines);
}

}  // namespace bmk
