// bedline.inc — what the BED line parsers of the offline commands share (plain C++: part of offline.hip through siteperf.inc, bedmerge.inc and
// bsperf.inc, and compiled by g++ as it stands through them: tests/*_asan_driver.cpp).  A field is a run of printable bytes (0x21 - 0x7e), a
// separator is ' ' or '\t'; a number is 1 - 10 digits with a value <= 2^31 - 1; a strand is the one byte '+' or '-'; a name is compared byte for
// byte.  The grammars differ (siteperf.inc: exactly one separator, >= 12 fields; bedmerge.inc: runs of separators, >= 12 fields; bsperf.inc:
// runs, exactly 11 fields, line classes) and are stated in those files on these routines; none of them reads outside p[0 .. n).
// for_each_line is the host's walk over a text, for every parser that has a host side (the .xy rows of xyparse.hip.inc included).
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define BED_HD __host__ __device__
#else
#define BED_HD
#endif

namespace bed {

constexpr int MAX_NAME = 255;

struct Name {
    char s[MAX_NAME + 1];
    int n;
};

// a name of 1 to MAX_NAME bytes -> name; false: null, empty or longer
inline bool set_name(Name& name, const char* contig_name) {
    const size_t n = contig_name ? std::strlen(contig_name) : 0;
    if (n < 1 || n > size_t(MAX_NAME)) return false;
    std::memset(name.s, 0, sizeof name.s);
    std::memcpy(name.s, contig_name, n);
    name.n = int(n);
    return true;
}

// every byte of s[0 .. n) is one a field can hold
BED_HD inline bool printable(const char* s, const long long n) {
    for (long long j = 0; j < n; ++j)
        if ((unsigned char)s[j] < 0x21 || (unsigned char)s[j] > 0x7e) return false;
    return true;
}

BED_HD inline bool is_sep(const char c) { return c == ' ' || c == '\t'; }

// i -> behind the run of separators at p[i] (i itself if there is none)
BED_HD inline void skip_seps(const char* p, const long long n, long long& i) {
    while (i < n && is_sep(p[i])) ++i;
}

enum { F_FIELD, F_NONE, F_BAD };

// The field that starts at p[i] -> F_FIELD: it is p[b .. b + len), and i is behind it (on a separator, or n); F_NONE: no field starts at i (i is n
// or on a separator; len = 0); F_BAD: a byte that is neither printable nor a separator.  Separators are the caller's: stepping over exactly one
// of them or over a run (skip_seps) is what tells the grammars apart.
BED_HD inline int next_field(const char* p, const long long n, long long& i, long long& b, long long& len) {
    for (b = i; i < n && !is_sep(p[i]); ++i)
        if ((unsigned char)p[i] < 0x21 || (unsigned char)p[i] > 0x7e) return F_BAD;
    len = i - b;
    return len ? F_FIELD : F_NONE;
}

// p[b .. e): 1 - 10 digits with a value <= 2^31 - 1 -> v
BED_HD inline bool parse_u31(const char* p, const long long b, const long long e, long long& v) {
    if (e - b < 1 || e - b > 10) return false;
    v = 0;
    for (long long j = b; j < e; ++j) {
        if (p[j] < '0' || p[j] > '9') return false;
        v = v * 10 + (p[j] - '0');
    }
    return v <= 0x7fffffffLL;
}

// the field p[b .. b + len) is '+' (s = 0) or '-' (s = 1)
BED_HD inline bool strand_of(const char* p, const long long b, const long long len, unsigned char& s) {
    if (len != 1 || (p[b] != '+' && p[b] != '-')) return false;
    s = p[b] == '-' ? 1 : 0;
    return true;
}

// the field p[b .. b + len) is name[0 .. name_len), byte for byte
BED_HD inline bool same_bytes(const char* p, const long long b, const long long len, const char* name, const int name_len) {
    if (len != name_len) return false;
    for (int j = 0; j < name_len; ++j)
        if (p[b + j] != name[j]) return false;
    return true;
}

// The text [0, n_bytes) line by line, a last line without '\n' ending with the text: fn(line, its length without the '\n', its 0-based index) ->
// the line is inside the grammar.  -> lines; *bad: the first line fn refused (1-based), 0: none.
template <class Fn>
inline int64_t for_each_line(const char* text, const int64_t n_bytes, int64_t* bad, Fn&& fn) {
    int64_t rows = 0;
    *bad = 0;
    for (int64_t b = 0; b < n_bytes; ++rows) {
        const void* nl = std::memchr(text + b, '\n', size_t(n_bytes - b));
        const int64_t e = nl ? static_cast<const char*>(nl) - text : n_bytes;
        if (!fn(text + b, e - b, rows) && *bad == 0) *bad = rows + 1;
        b = e + 1;
    }
    return rows;
}

}  // namespace bed
