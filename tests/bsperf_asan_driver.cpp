// TEST INFRASTRUCTURE - not part of the product.  The line routine of `bsperf` (deepmod_amd/csrc/bsperf.inc: bsk::parse_line / parse_text, the code the
// kernel of bsperf.hip.inc runs) under -fsanitize=address,undefined, as a program.  Every text and every record array lives in a heap block of exactly its
// size, so that a read or a write one byte outside it is a sanitizer report.  Texts cut at every byte (truncated last lines, a missing final '\n'),
// with and without the first-line skip, against a plain restatement of the rules; every violation with its line number; record capacities one short.
// tests/test_bsperf_host.py builds and runs it.
#include "../deepmod_amd/csrc/bsperf.inc"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

namespace {

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

struct Parsed {
    int64_t recs = 0, bad = 0;
    std::vector<int64_t> lines;
    std::vector<int32_t> pos;
    std::vector<uint32_t> meta;
};

const char* const kNames[] = {"chr1", "chr10", "chrX"};

// the text in a block of exactly its size; the records in blocks of exactly `recs` elements (sized by a first call with cap 0), then with a
// capacity one short: the last record is not written
Parsed parse(const std::string& text, bool first_chunk, const int64_t* lengths = nullptr) {
    bsk::Names names;
    CHECK(bsk::set_names(names, 3, kNames, lengths) == 0);
    std::unique_ptr<char[]> t(new char[text.size()]);
    std::copy(text.begin(), text.end(), t.get());
    Parsed r;
    r.lines.assign(bsk::N_LINE, 0);
    r.recs = bsk::parse_text(t.get(), int64_t(text.size()), names, first_chunk, nullptr, nullptr, 0, r.lines.data(), &r.bad);
    std::unique_ptr<int32_t[]> pos(new int32_t[size_t(r.recs)]);
    std::unique_ptr<uint32_t[]> meta(new uint32_t[size_t(r.recs)]);
    int64_t bad2 = -1;
    std::vector<int64_t> lines2(bsk::N_LINE, -1);
    CHECK(bsk::parse_text(t.get(), int64_t(text.size()), names, first_chunk, pos.get(), meta.get(), r.recs, lines2.data(), &bad2) == r.recs && bad2 == r.bad && lines2 == r.lines);
    r.pos.assign(pos.get(), pos.get() + r.recs);
    r.meta.assign(meta.get(), meta.get() + r.recs);
    if (r.recs > 0) {
        std::unique_ptr<int32_t[]> pos1(new int32_t[size_t(r.recs - 1)]);
        std::unique_ptr<uint32_t[]> meta1(new uint32_t[size_t(r.recs - 1)]);
        CHECK(bsk::parse_text(t.get(), int64_t(text.size()), names, first_chunk, pos1.get(), meta1.get(), r.recs - 1, lines2.data(), &bad2) == r.recs);
        CHECK(std::equal(pos1.get(), pos1.get() + r.recs - 1, r.pos.begin()) && std::equal(meta1.get(), meta1.get() + r.recs - 1, r.meta.begin()));
    }
    return r;
}

// Python's line.split() on a line of printable bytes, blanks and tabs
std::vector<std::string> split(const std::string& line) {
    std::vector<std::string> out;
    std::istringstream in(line);
    std::string f;
    while (in >> f) out.push_back(f);
    return out;
}

bool number(const std::string& f, long long& v) {
    if (f.empty() || f.size() > 10 || f.find_first_not_of("0123456789") != std::string::npos) return false;
    v = std::stoll(f);
    return v <= 2147483647LL;
}

// the class of one line by the rules as the issue states them
int restated(const std::string& raw, Parsed* into) {
    size_t lo = raw.find_first_not_of(" \t"), hi = raw.find_last_not_of(" \t");
    const std::string line = lo == std::string::npos ? "" : raw.substr(lo, hi - lo + 1);
    if (line.size() <= 20) return bsk::L_SHORT;
    for (unsigned char c : line)
        if (c != ' ' && c != '\t' && (c < 0x21 || c > 0x7e)) return bsk::L_BAD;
    const std::vector<std::string> f = split(line);
    long long p = 0, cv = 0, pc = 0;
    if (f.size() != 11 || !number(f[1], p) || !number(f[9], cv) || !number(f[10], pc) || pc > 100) return bsk::L_BAD;
    if (f[5] != "+" && f[5] != "-") return bsk::L_STRAND;
    int c = -1;
    for (int k = 0; k < 3; ++k)
        if (f[0] == kNames[k]) c = k;
    if (c < 0) return bsk::L_CONTIG;
    if (p >= bsk::MAX_LENGTH) return bsk::L_BAD;
    if (cv == 0) return bsk::L_ZERO;
    if (into) {
        into->pos.push_back(int32_t(p));
        into->meta.push_back(uint32_t(std::min<long long>(cv, 65535)) | uint32_t(pc) << 16 | uint32_t(f[5] == "-") << 23 | uint32_t(c) << 24);
    }
    return bsk::L_RECORD;
}

}  // namespace

int main() {
    const std::string header = "chrom start end name score strand thickStart thickEnd rgb coverage percentage\n",
                      tabs = "chr1\t1005\t1006\t.\t33\t+\t1005\t1006\t0,0,0\t33\t91\n", blanks = "chr10 7 8 . 5 - 7 8 0,0,0 70000 0 \n",
                      mixed = " \tchrX\t0  1 .\t\t1 - 0 1 0,0,0 \t2147483647 100\t \n", other = "chr11 7 8 . 5 - 7 8 0,0,0 5 0\n", dot = "chr1 7 8 . 5 . 7 8 0,0,0 5 0\n",
                      zero = "chr1 9 10 . 0 + 9 10 0,0,0 0 0\n", brief = "chr1 1 2 . 1 +\n", blank = " \t \n";
    const std::string whole = header + tabs + blanks + mixed + other + dot + zero + brief + blank + tabs;
    Parsed r = parse(whole, true);
    CHECK(r.bad == 0 && r.recs == 4 && r.lines == (std::vector<int64_t>{4, 1, 2, 1, 1, 1}));
    CHECK(r.pos == (std::vector<int32_t>{1005, 7, 0, 1005}));
    CHECK(r.meta == (std::vector<uint32_t>{33u | 91u << 16, 65535u | 1u << 23 | 1u << 24, 65535u | 100u << 16 | 1u << 23 | 2u << 24, 33u | 91u << 16}));
    // a text cut at every byte, as the first chunk of a file and as a later one: nothing behind the cut is read, and every line has the class of the restatement
    for (int first = 0; first < 2; ++first)
        for (size_t cut = 0; cut <= whole.size(); ++cut) {
            const std::string text = whole.substr(0, cut);
            r = parse(text, first != 0);
            Parsed want;
            want.lines.assign(bsk::N_LINE, 0);
            int64_t no = 0;
            for (size_t b = 0; b < text.size();) {
                size_t e = text.find('\n', b);
                if (e == std::string::npos) e = text.size();
                ++no;
                const int cls = (first && no == 1) ? int(bsk::L_HEADER) : restated(text.substr(b, e - b), &want);
                if (cls == bsk::L_BAD) {
                    if (!want.bad) want.bad = no;
                } else {
                    ++want.lines[size_t(cls)];
                }
                b = e + 1;
            }
            CHECK(r.bad == want.bad && r.lines == want.lines && r.pos == want.pos && r.meta == want.meta && r.recs == int64_t(want.pos.size()));
        }
    // every violation, as line 3 of four (behind the first line of the file) and as a last line without '\n'
    const char* bad_lines[] = {
        "chr1 5 6 . 7 + 5 6 0,0,0 42",                   // 10 fields
        "chr1 5 6 . 7 + 5 6 0,0,0 7 42 3",               // 12 fields
        "chr1 5 6 . 7 + 5 6 0,0,0 7 42\r",               // '\r'
        "chr1 +5 6 . 7 + 5 6 0,0,0 7 42",                // a sign
        "chr1 5 6 . 7 + 5 6 0,0,0 -7 42",
        "chr1 5 6 . 7 + 5 6 0,0,0 7 +42",
        "chr1 5 6 . 7 + 5 6 0,0,0 00000000007 42",       // 11 digits
        "chr1 5 6 . 7 + 5 6 0,0,0 2147483648 42",        // above 2^31 - 1
        "chr1 2147483647 6 . 7 + 5 6 0,0,0 7 42",        // position + 1 is no int32
        "chr1 5 6 . 7 + 5 6 0,0,0 7 101",                // percentage 101
        "chr1 5 6 . 7 + 5 6 0,0,0 7 4x",
        "chr1 5 6 . 7 + 5 6 0,0,0 7 42 \x01",            // a byte that is neither printable nor a separator
        "chr1 5 6 . 7 + 5 6 0,0,0 7 42\v",
        "chr7 5 6 . 7 + 5 6 0,0,0 7 101",                // of a contig that is not requested: the grammar comes first
    };
    for (const char* line : bad_lines) {
        r = parse(header + tabs + line + "\n" + blanks, true);
        CHECK(r.bad == 3 && r.lines[bsk::L_RECORD] == 2);
        r = parse(tabs + line, false);
        CHECK(r.bad == 2 && r.recs == 1);
        r = parse(std::string(line) + "\n" + tabs, true);    // as the first line of a file it is skipped unread
        CHECK(r.bad == 0 && r.recs == 1);
    }
    const int64_t lengths[3] = {1006, 7, -1};                // a position at or beyond the contig's length
    r = parse(header + tabs + blanks, true, lengths);
    CHECK(r.bad == 3 && r.lines[bsk::L_RECORD] == 1);
    const int64_t lengths2[3] = {1006, 8, -1};
    r = parse(header + tabs + blanks, true, lengths2);
    CHECK(r.bad == 0 && r.recs == 2);
    r = parse(std::string("chr1 5 6 . 7 + 5 6 0,0,0 7 42\0\n", 31), false);      // a NUL byte
    CHECK(r.bad == 1);
    // names: 1 to 64 distinct names of 1 to 63 printable bytes, lengths of 1 to 2^31 - 1
    bsk::Names nm;
    const std::string k63(63, 'k'), k64(64, 'k');
    const char* ok[] = {k63.c_str()};
    const char* too_long[] = {k64.c_str()};
    const char* twice[] = {"a", "b", "a"};
    const char* blank_in[] = {"a b"};
    const char* empty[] = {""};
    const int64_t zero_len[1] = {0}, huge[1] = {2147483648LL};
    CHECK(bsk::set_names(nm, 1, ok, nullptr) == 0 && nm.n == 1 && nm.len[0] == 63 && nm.limit[0] == bsk::MAX_LENGTH);
    CHECK(bsk::set_names(nm, 1, too_long, nullptr) == 1 && bsk::set_names(nm, 3, twice, nullptr) == 3 && bsk::set_names(nm, 1, blank_in, nullptr) == 1 &&
          bsk::set_names(nm, 1, empty, nullptr) == 1 && bsk::set_names(nm, 0, ok, nullptr) != 0 && bsk::set_names(nm, 65, ok, nullptr) != 0 &&
          bsk::set_names(nm, 1, ok, zero_len) == 1 && bsk::set_names(nm, 1, ok, huge) == 1 && bsk::set_names(nm, 1, nullptr, nullptr) != 0);
    std::vector<std::string> many;
    std::vector<const char*> many_p;
    for (int k = 0; k < 64; ++k) many.push_back("contig_" + std::to_string(k));
    for (const std::string& s : many) many_p.push_back(s.c_str());
    CHECK(bsk::set_names(nm, 64, many_p.data(), nullptr) == 0);
    {
        const std::string text = "contig_63 5 6 . 7 - 5 6 0,0,0 7 42\ncontig_6 5 6 . 7 + 5 6 0,0,0 7 42\ncontig_64 5 6 . 7 + 5 6 0,0,0 7 42\n";
        std::unique_ptr<char[]> t(new char[text.size()]);
        std::copy(text.begin(), text.end(), t.get());
        int32_t pos[2];
        uint32_t meta[2];
        int64_t lines[bsk::N_LINE], bad = -1;
        CHECK(bsk::parse_text(t.get(), int64_t(text.size()), nm, false, pos, meta, 2, lines, &bad) == 2 && bad == 0 && lines[bsk::L_CONTIG] == 1);
        CHECK(bsk::meta_contig(meta[0]) == 63 && bsk::meta_strand(meta[0]) == 1 && bsk::meta_contig(meta[1]) == 6 && bsk::meta_cov(meta[1]) == 7 && bsk::meta_pct(meta[1]) == 42);
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("BSPERF-ASAN-OK\n");
    return 0;
}
