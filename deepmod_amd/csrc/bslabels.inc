// bslabels.inc — `bslabels`, the class rule and the line routine (plain C++: part of offline.hip through bslabels.hip.inc, and compiled by g++ as it
// stands: tests/bslabels_asan_driver.cpp).  The kernels of bslabels.hip.inc and the host entry point dm_bslabels_format_host run these routines,
// so the device and the host cannot disagree on a class or on a line.
//
// The class of a key (strand, position) of the open contig (class_of), from its R truth slots (bsperf.hip.inc: 0 no record, else PRESENT |
// percentage << 16 | coverage, the coverage saturated at 65,535) and the site bit of its strand:
//   C_NONE  no replicate has a record
//   C_OFF   a record somewhere, but the motif does not lie on that strand with its modified base at that position
//   C_FUL   every replicate has a record, the smallest coverage is >= cov and every percentage is >= methylated
//   C_NO    every replicate has a record, the smallest coverage is >= cov and every percentage is <= unmethylated
//   C_ANY   every other admissible key with a record: partial methylation, replicates that disagree, low coverage, a key missing from a replicate
// unmethylated < methylated, so no key is both C_FUL and C_NO: the lists are disjoint.
//
// A line of a list (emit_line): '%s %s %d\n' % (chr, strand, pos), the `chr strand pos` line getfeatures.readPosFiles reads; pos is the 0-based
// position (the bedMethyl start), 1 - 10 digits.  Ascending position, '+' before '-' at one position (emit_position).
#pragma once
#include "bedline.inc"
#include "textout.inc"

#define BL_HD BED_HD

namespace blk {

using bed::Name;
constexpr long long MAX_LENGTH = 0x7fffffffLL;      // positions 0 .. 2^31 - 2
constexpr int MAX_MOTIF = 8;
constexpr int MAX_REP = 4;
constexpr unsigned PRESENT = 0x80000000u;           // a truth slot with a record (bsk::PRESENT)
enum { C_NONE, C_FUL, C_ANY, C_NO, C_OFF, N_CLASS };
enum { N_FUL, N_ANY, N_NO, N_OFF, N_BARE, N_COUNT };                 // the counters of a strand: the four classes, admissible sites without truth

struct Rule {
    int n_rep, cov, methylated, unmethylated;
};

// slot[r * stride]: the slot of replicate r; admissible: the site bit of the key's strand
BL_HD inline int class_of(const unsigned* slot, const long long stride, const Rule& p, const bool admissible) {
    bool any = false, all = true, all_high = true, all_low = true;
    int m = 0x7fffffff;
    for (int r = 0; r < p.n_rep; ++r) {
        const unsigned v = slot[(long long)r * stride];
        any = any || v != 0;
        all = all && v != 0;
        const int pct = int((v >> 16) & 0x7fu), cv = int(v & 0xffffu);
        m = cv < m ? cv : m;
        all_high = all_high && pct >= p.methylated;
        all_low = all_low && pct <= p.unmethylated;
    }
    if (!any) return C_NONE;
    if (!admissible) return C_OFF;
    if (all && m >= p.cov && all_high) return C_FUL;
    if (all && m >= p.cov && all_low) return C_NO;
    return C_ANY;
}

// The same routine counts and writes: the two cannot disagree on a length.
template <class Sink>
BL_HD inline void emit_line(Sink& s, const Name& name, const int strand, const long long pos) {
    for (int j = 0; j < name.n; ++j) s.put(name.s[j]);
    s.put(' ');
    s.put(strand ? '-' : '+');
    s.put(' ');
    txo::put_uint(s, (unsigned long long)pos);
    s.put('\n');
}

// The lines of position q (index i of the class arrays; a null strand holds nothing) in list `list` (C_FUL, C_ANY or C_NO): '+' first.  -> lines emitted
template <class Sink>
BL_HD inline int emit_position(Sink& s, const Name& name, const int list, const long long q, const long long i, const unsigned char* cls_p, const unsigned char* cls_m) {
    int lines = 0;
    if (cls_p && cls_p[i] == list) {
        emit_line(s, name, 0, q);
        ++lines;
    }
    if (cls_m && cls_m[i] == list) {
        emit_line(s, name, 1, q);
        ++lines;
    }
    return lines;
}

// a contig name for `bslabels`: 1 to bsk::MAX_NAME (63) printable bytes, as dm_bslabels_create takes them
inline bool set_name(Name& name, const char* contig_name) { return bed::set_name(name, contig_name) && name.n <= 63 && bed::printable(name.s, name.n); }

// The lines of list `list` as an emitter (textout.inc): the class arrays of the two strands, a null strand holds nothing
struct Emitter {
    Name name;
    int list;
    const unsigned char *cls_p, *cls_m;
    static constexpr bool CHECKED = false;
    template <class Sink>
    BL_HD int operator()(Sink& s, const long long q, const long long i) const {
        return emit_position(s, name, list, q, i, cls_p, cls_m);
    }
};

// The text of list `list` for positions first_pos .. first_pos + length - 1 from the two class arrays: counted first; written only if it fits `cap`.
// -> bytes of the text
inline int64_t format_classes(const Name& name, const int list, const int64_t first_pos, const int64_t length, const unsigned char* cls_p, const unsigned char* cls_m, char* out,
                              const int64_t cap, int64_t* lines) {
    return txo::format_range(Emitter{name, list, cls_p, cls_m}, first_pos, length, out, cap, lines);
}

}  // namespace blk
