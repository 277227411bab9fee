// bedtext.inc — BED text of one contig x strand from the dense counters (host code, part of summary.hip).
//
// Reference: /root/reference/bin/DeepMod_scripts/myDetect.py:1107-1120 (sum_handler's writer): for every key that was
// created (touch > 0), in position order,
//     "<chr> <pos> <pos+1> <Base> <min(cov,1000)> <strand> <pos> <pos+1> 0,0,0 <cov> <pct> <mod> \n"
// single spaces, a trailing space before the newline, pct = "%d" % (100 * mod / (cov if cov > 0 else 1)) (truncation).
// A 30x E. coli run has 2.3 M such lines, a human chromosome 1e8: formatted here instead of in a Python loop.
#pragma once
#include "host.h"

namespace bedtext {
// decimal digits of v, two at a time from a 00..99 table
inline char* put_u64(char* p, unsigned long long v) {
    static const char D[201] =
        "0001020304050607080910111213141516171819202122232425262728293031323334353637383940414243444546474849"
        "5051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
    char tmp[24];
    int n = 0;
    while (v >= 100) {
        const unsigned r = unsigned(v % 100);
        v /= 100;
        tmp[n++] = D[2 * r + 1];
        tmp[n++] = D[2 * r];
    }
    if (v >= 10) {
        tmp[n++] = D[2 * v + 1];
        tmp[n++] = D[2 * v];
    } else {
        tmp[n++] = char('0' + v);
    }
    while (n) *p++ = tmp[--n];
    return p;
}
constexpr int64_t LINE_EXTRA = 128;      // upper bound of a line's bytes beyond the contig name (6 numbers of <= 20 digits are never reached: positions < 2^33)
}  // namespace bedtext

extern "C" {

// Writes the text into out (capacity cap) and returns its length in bytes.  With out == NULL (or a capacity below the safe bound
// lines * (strlen(chrom) + 128)) nothing is written and that bound is returned: allocate it and call again.
// dm_bed_format_at: the counters are those of positions [first_pos, first_pos + length) (a rank's slice after dm_summary_reduce_scatter).
int64_t dm_bed_format_at(const char* chrom, char strand, char base, int64_t first_pos, const int32_t* touch, const int32_t* cov, const int32_t* mod,
                         int64_t length, char* out, int64_t cap) {
    if (!chrom || length < 0 || first_pos < 0 || (length > 0 && (!touch || !cov || !mod))) return fail(DM_EINVAL, "dm_bed_format: bad input");
    const size_t nchr = std::strlen(chrom);
    int64_t lines = 0;
    for (int64_t i = 0; i < length; ++i) lines += touch[i] > 0;
    const int64_t bound = lines * int64_t(nchr + bedtext::LINE_EXTRA);
    if (!out || cap < bound) return bound;
    char* w = out;
    for (int64_t i = 0; i < length; ++i) {
        if (touch[i] <= 0) continue;
        const unsigned long long p = (unsigned long long)(first_pos + i);
        const long long cv = cov[i], md = mod[i];
        std::memcpy(w, chrom, nchr);
        w += nchr;
        *w++ = ' ';
        w = bedtext::put_u64(w, p);
        *w++ = ' ';
        w = bedtext::put_u64(w, p + 1);
        *w++ = ' ';
        *w++ = base;
        *w++ = ' ';
        w = bedtext::put_u64(w, (unsigned long long)(cv > 1000 ? 1000 : cv));
        *w++ = ' ';
        *w++ = strand;
        *w++ = ' ';
        w = bedtext::put_u64(w, p);
        *w++ = ' ';
        w = bedtext::put_u64(w, p + 1);
        std::memcpy(w, " 0,0,0 ", 7);
        w += 7;
        w = bedtext::put_u64(w, (unsigned long long)cv);
        *w++ = ' ';
        w = bedtext::put_u64(w, (unsigned long long)(100 * md / (cv > 0 ? cv : 1)));
        *w++ = ' ';
        w = bedtext::put_u64(w, (unsigned long long)md);
        *w++ = ' ';
        *w++ = '\n';
    }
    return int64_t(w - out);
}

int64_t dm_bed_format(const char* chrom, char strand, char base, const int32_t* touch, const int32_t* cov, const int32_t* mod,
                      int64_t length, char* out, int64_t cap) {
    return dm_bed_format_at(chrom, strand, base, 0, touch, cov, mod, length, out, cap);
}

// The lines of hm_cluster_predict.py's output for n sites of one strand (the records of dm_cluster_sites_fetch): the row sum_chr_mod.py:63
// writes - "<chr> <pos> <pos+1> <Base> <min(cov,1000)> <strand>  <pos> <pos+1> 0,0,0 <cov> <int(mod*100/cov)> <mod>", two spaces after the
// strand, no trailing space - then " <new>\n" (hm_cluster_predict.py:170).  Sized first like dm_bed_format_at: bound = n * (strlen(chrom) + 128).
int64_t dm_cluster_bed_format(const char* chrom, char strand, char base, const int64_t* pos, const int32_t* cov, const int32_t* mod, const int32_t* new_pct,
                              int64_t n, char* out, int64_t cap) {
    if (!chrom || n < 0 || (n > 0 && (!pos || !cov || !mod || !new_pct))) return fail(DM_EINVAL, "dm_cluster_bed_format: bad input");
    for (int64_t i = 0; i < n; ++i)
        if (pos[i] < 0 || pos[i] >= (int64_t(1) << 40) || cov[i] < 0 || mod[i] < 0 || new_pct[i] < 0)      // (13-digit positions: a line stays below the bound)
            return fail(DM_EINVAL, "dm_cluster_bed_format: value out of range in record %lld", (long long)i);
    const size_t nchr = std::strlen(chrom);
    const int64_t bound = n * int64_t(nchr + bedtext::LINE_EXTRA);
    if (!out || cap < bound) return bound;
    char* w = out;
    for (int64_t i = 0; i < n; ++i) {
        const unsigned long long p = (unsigned long long)pos[i];
        const long long cv = cov[i], md = mod[i];
        std::memcpy(w, chrom, nchr);
        w += nchr;
        *w++ = ' ';
        w = bedtext::put_u64(w, p);
        *w++ = ' ';
        w = bedtext::put_u64(w, p + 1);
        *w++ = ' ';
        *w++ = base;
        *w++ = ' ';
        w = bedtext::put_u64(w, (unsigned long long)(cv < 1000 ? cv : 1000));
        *w++ = ' ';
        *w++ = strand;
        *w++ = ' ';
        *w++ = ' ';
        w = bedtext::put_u64(w, p);
        *w++ = ' ';
        w = bedtext::put_u64(w, p + 1);
        std::memcpy(w, " 0,0,0 ", 7);
        w += 7;
        w = bedtext::put_u64(w, (unsigned long long)cv);
        *w++ = ' ';
        w = bedtext::put_u64(w, (unsigned long long)(cv > 0 ? md * 100 / cv : 0));
        *w++ = ' ';
        w = bedtext::put_u64(w, (unsigned long long)md);
        *w++ = ' ';
        w = bedtext::put_u64(w, (unsigned long long)new_pct[i]);
        *w++ = '\n';
    }
    return int64_t(w - out);
}

}  // extern "C"
