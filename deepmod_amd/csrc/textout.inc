// textout.inc — what the text writers of the offline commands share (plain C++: part of offline.hip through bedmerge.inc, bslabels.inc and
// xyrows.hip.inc, and compiled by g++ as it stands through the first two: tests/*_asan_driver.cpp).  A line routine is a template on a sink and
// puts its bytes one by one: with the counting sink it gives the length of its text, with the writing sink the text, so the two cannot disagree.
// An emitter is a small trivially copyable struct that holds what a command's lines are made of (the contig's name, its tables) and has one call
//     template <class Sink> int operator()(Sink& s, long long q, long long i) const    the lines of position q, index i of its arrays -> lines emitted
// format_range runs one on the host; the kernels of textout.hip.inc run the same emitter per tile.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TXO_HD __host__ __device__
#else
#define TXO_HD
#endif

namespace txo {

struct CountSink {
    long long n = 0;
    TXO_HD void put(char) { ++n; }
};
struct WriteSink {
    char* p;
    TXO_HD void put(const char c) { *p++ = c; }
};

template <class Sink, class U>
TXO_HD inline void put_uint(Sink& s, U v) {                          // the decimal digits of v, most significant first, without a digit buffer
    U p = 1;
    while (p <= v / 10) p *= 10;
    while (p) {
        const U d = v / p;
        s.put(char('0' + int(d)));
        v -= d * p;
        p /= 10;
    }
}

// The text of positions first_pos .. first_pos + length - 1 (indices 0 .. length - 1 of the emitter's arrays): counted first; written only if
// it fits `cap`.  -> bytes of the text; *lines: its lines
template <class Emitter>
inline int64_t format_range(const Emitter& em, const int64_t first_pos, const int64_t length, char* out, const int64_t cap, int64_t* lines) {
    CountSink count;
    int64_t n_lines = 0;
    for (int64_t i = 0; i < length; ++i) n_lines += em(count, first_pos + i, i);
    if (lines) *lines = n_lines;
    if (out && cap >= count.n) {
        WriteSink w{out};
        for (int64_t i = 0; i < length; ++i) em(w, first_pos + i, i);
    }
    return count.n;
}

}  // namespace txo
