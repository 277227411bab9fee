// TEST INFRASTRUCTURE - not part of the product.  The line routines of `merge` (deepmod_amd/csrc/bedmerge.inc: bmk::parse_line / parse_text, the device
// grammar, and bmk::emit_line / format_tables, the merged dialect - the code the kernels of bedmerge.hip.inc run) under -fsanitize=address,undefined, as a
// program.  Every text, every record array, every table and every output lives in a heap block of exactly its size, so that a read or a write one byte
// outside it is a sanitizer report.  Texts cut at every byte (truncated last lines, a missing final '\n'), the dialects against a plain restatement,
// every violation with its line number, the formatter against snprintf, a capacity one byte short.  tests/test_merge_host.py builds and runs it.
#include "../deepmod_amd/csrc/bedmerge.inc"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
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

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a block of exactly v.size() elements (new T[0] is a valid, unreadable block)
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

struct Parsed {
    int64_t rows = 0, bad = 0;
    std::vector<int32_t> pos, cov, mod;
    std::vector<uint8_t> strand;
};

// the text in a block of exactly its size; the records in blocks of exactly `rows` elements (sized by a first call with cap 0)
Parsed parse(const std::string& text, const char* contig, long long limit = bmk::MAX_LENGTH) {
    bmk::Name name;
    CHECK(bmk::set_name(name, contig));
    std::unique_ptr<char[]> t(new char[text.size()]);
    std::copy(text.begin(), text.end(), t.get());
    Parsed r;
    r.rows = bmk::parse_text(t.get(), int64_t(text.size()), name, limit, nullptr, nullptr, nullptr, nullptr, 0, &r.bad);
    std::unique_ptr<int32_t[]> pos(new int32_t[size_t(r.rows)]), cov(new int32_t[size_t(r.rows)]), mod(new int32_t[size_t(r.rows)]);
    std::unique_ptr<uint8_t[]> strand(new uint8_t[size_t(r.rows)]);
    int64_t bad2 = -1;
    CHECK(bmk::parse_text(t.get(), int64_t(text.size()), name, limit, pos.get(), strand.get(), cov.get(), mod.get(), r.rows, &bad2) == r.rows && bad2 == r.bad);
    r.pos.assign(pos.get(), pos.get() + r.rows);
    r.cov.assign(cov.get(), cov.get() + r.rows);
    r.mod.assign(mod.get(), mod.get() + r.rows);
    r.strand.assign(strand.get(), strand.get() + r.rows);
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

struct Tables {
    std::vector<int32_t> cp, mp, cm, mm;
};

// sum_chr_mod.py:63 by snprintf
std::string restated(const std::string& chrom, char base, int64_t first, const Tables& t) {
    std::string out;
    char buf[700];
    for (size_t i = 0; i < t.cp.size(); ++i)
        for (int s = 0; s < 2; ++s) {
            const int64_t cv = s ? t.cm[i] : t.cp[i], md = s ? t.mm[i] : t.mp[i], p = first + int64_t(i);
            if (md <= 0) continue;
            std::snprintf(buf, sizeof buf, "%s %" PRId64 " %" PRId64 " %c %" PRId64 " %c  %" PRId64 " %" PRId64 " 0,0,0 %" PRId64 " %" PRId64 " %" PRId64 "\n", chrom.c_str(), p,
                          p + 1, base, cv < 1000 ? cv : 1000, s ? '-' : '+', p, p + 1, cv, cv > 0 ? md * 100 / cv : 0, md);
            out += buf;
        }
    return out;
}

// sized by a call without output, then written into a block of exactly that size; a capacity one byte short writes nothing
std::string format(const std::string& chrom, char base, int64_t first, const Tables& t, bool minus_only = false) {
    bmk::Name name;
    CHECK(bmk::set_name(name, chrom.c_str()));
    auto cp = exact(t.cp), mp = exact(t.mp), cm = exact(t.cm), mm = exact(t.mm);
    const int32_t *pcp = minus_only ? nullptr : cp.get(), *pmp = minus_only ? nullptr : mp.get();
    const int64_t n = int64_t(t.cp.size());
    int64_t lines = -1, bad = -1;
    const int64_t need = bmk::format_tables(name, base, first, n, pcp, pmp, cm.get(), mm.get(), nullptr, 0, &lines, &bad);
    CHECK(need >= 0);
    if (need < 0) return "";
    if (need > 0) {
        std::unique_ptr<char[]> small(new char[size_t(need - 1)]);
        std::fill(small.get(), small.get() + need - 1, '#');
        CHECK(bmk::format_tables(name, base, first, n, pcp, pmp, cm.get(), mm.get(), small.get(), need - 1, &lines, &bad) == need);
        CHECK(std::count(small.get(), small.get() + need - 1, '#') == need - 1);
    }
    std::unique_ptr<char[]> out(new char[size_t(need)]);
    CHECK(bmk::format_tables(name, base, first, n, pcp, pmp, cm.get(), mm.get(), out.get(), need, &lines, &bad) == need);
    const std::string text(out.get(), out.get() + need);
    CHECK(lines == std::count(text.begin(), text.end(), '\n'));
    return text;
}

}  // namespace

int main() {
    // the three dialects and mixed separators
    const std::string detect = "chr1 1005 1006 C 33 + 1005 1006 0,0,0 33 24 8 \n", merged = "chr1 1005 1006 C 47 -  1005 1006 0,0,0 47 34 16\n",
                      clustered = "chr1 7 8 C 1000 +  7 8 0,0,0 1500 46 700 61\n", mixed = " \tchr1\t0  1 C\t\t1 - 0 1 0,0,0 \t2147483647 0 2147483647\t \n";
    Parsed r = parse(detect + merged + clustered + mixed, "chr1");
    CHECK(r.rows == 4 && r.bad == 0);
    CHECK(r.pos == (std::vector<int32_t>{1005, 1005, 7, 0}) && r.cov == (std::vector<int32_t>{33, 47, 1500, 2147483647}) &&
          r.mod == (std::vector<int32_t>{8, 16, 700, 2147483647}) && r.strand == (std::vector<uint8_t>{0, 1, 0, 1}));
    // a text cut at every byte: the last line is truncated or lacks its '\n'; nothing behind the cut is read, and the verdict on the last line is
    // that of a plain restatement (12 fields, numeric fields of 1 - 10 digits)
    const std::string whole = detect + merged + clustered + mixed;
    for (size_t cut = 0; cut <= whole.size(); ++cut) {
        const std::string text = whole.substr(0, cut);
        r = parse(text, "chr1");
        const int64_t want_rows = std::count(text.begin(), text.end(), '\n') + ((!text.empty() && text.back() != '\n') ? 1 : 0);
        CHECK(r.rows == want_rows);
        bool last_ok = true;
        if (!text.empty() && text.back() != '\n') {
            const size_t b = text.rfind('\n');
            const std::vector<std::string> f = split(text.substr(b == std::string::npos ? 0 : b + 1));
            last_ok = f.size() >= 12 && f[0] == "chr1";
            if (last_ok)
                for (int k : {1, 9, 11}) last_ok = last_ok && !f[size_t(k)].empty() && f[size_t(k)].size() <= 10 && f[size_t(k)].find_first_not_of("0123456789") == std::string::npos;
            if (last_ok) last_ok = (f[5] == "+" || f[5] == "-") && std::stoll(f[11]) <= std::stoll(f[9]) && std::stoll(f[9]) <= 2147483647LL && std::stoll(f[1]) < 2147483647LL;
        }
        CHECK(r.bad == (last_ok ? 0 : want_rows));
    }
    // every violation, as line 2 of three
    const char* bad_lines[] = {
        "chr1 5 6 C 7 + 5 6 0,0,0 7 42 3\r",             // '\r'
        "",                                              // a blank line
        "  \t ",                                         // blanks only
        "chr2 5 6 C 7 + 5 6 0,0,0 7 42 3",               // another contig
        "chr11 5 6 C 7 + 5 6 0,0,0 7 42 3",              // a longer name
        "chr 5 6 C 7 + 5 6 0,0,0 7 42 3",                // a shorter name
        "chr1 +5 6 C 7 + 5 6 0,0,0 7 42 3",              // a sign
        "chr1 5 6 C 7 + 5 6 0,0,0 -7 42 3",
        "chr1 5 6 C 7 + 5 6 0,0,0 7 42",                 // 11 fields
        "chr1 5 6 C 7 + 5 6 0,0,0 7 42 00000000003",     // 11 digits
        "chr1 5 6 C 7 + 5 6 0,0,0 2147483648 42 3",      // above 2^31 - 1
        "chr1 2147483647 6 C 7 + 5 6 0,0,0 7 42 3",      // position + 1 is no int32
        "chr1 5 6 C 7 * 5 6 0,0,0 7 42 3",               // strand
        "chr1 5 6 C 7 +- 5 6 0,0,0 7 42 3",
        "chr1 5 6 C 7 + 5 6 0,0,0 7 42 8",               // modified > coverage
        "chr1 5 6 C 7 + 5 6 0,0,0 7 42 3x",
        "chr1 5 6 C 7 + 5 6 0,0,0 7 42 3 \x01",          // a byte that is neither printable nor a separator, behind the twelfth field
        "chr1 5 6 C 7 + 5 6 0,0,0 7 42 3\v",
    };
    for (const char* line : bad_lines) {
        r = parse(detect + line + "\n" + merged, "chr1");
        CHECK(r.rows == 3 && r.bad == 2);
        r = parse(detect + merged + line, "chr1");           // as the last line, without '\n' (a blank one is then no line at all)
        CHECK(std::string(line).empty() ? (r.rows == 2 && r.bad == 0) : (r.rows == 3 && r.bad == 3));
    }
    r = parse("chr1 1004 1005 C 7 + 5 6 0,0,0 7 42 3\nchr1 1005 1006 C 7 + 5 6 0,0,0 7 42 3\n", "chr1", 1005);      // beyond the table
    CHECK(r.rows == 2 && r.bad == 2);
    r = parse(std::string("chr1 5 6 C 7 + 5 6 0,0,0 7 42 3\0\n", 33), "chr1");                                         // a NUL byte
    CHECK(r.rows == 1 && r.bad == 1);
    bmk::Name nm;
    CHECK(!bmk::set_name(nm, "") && !bmk::set_name(nm, nullptr) && !bmk::set_name(nm, std::string(256, 'k').c_str()) && !bmk::set_name(nm, "a b") &&
          bmk::set_name(nm, std::string(255, 'k').c_str()) && nm.n == 255);
    const std::string long_name(255, 'q');
    r = parse(long_name + " 5 6 C 7 + 5 6 0,0,0 7 42 3\n" + long_name.substr(1) + " 5 6 C 7 + 5 6 0,0,0 7 42 3", long_name.c_str());
    CHECK(r.rows == 2 && r.bad == 2 && r.pos[0] == 5);

    // ---- the formatter ----
    Tables t;
    CHECK(format("chr1", 'C', 0, t).empty());                                                       // no position
    t = {{7, 5, 0, 9}, {3, 0, 0, 9}, {0, 5, 1, 2}, {0, 5, 0, 1}};
    CHECK(format("chr1", 'C', 9, t) == "chr1 9 10 C 7 +  9 10 0,0,0 7 42 3\nchr1 10 11 C 5 -  10 11 0,0,0 5 100 5\nchr1 12 13 C 9 +  12 13 0,0,0 9 100 9\n"
                                       "chr1 12 13 C 2 -  12 13 0,0,0 2 50 1\n");
    CHECK(format("chr1", 'C', 9, t, true) == "chr1 10 11 C 5 -  10 11 0,0,0 5 100 5\nchr1 12 13 C 2 -  12 13 0,0,0 2 50 1\n");
    // digit-count steps of position and position + 1, the largest position, the coverage cap, every percentage
    for (int64_t p = 10; p <= 1000000000LL; p *= 10) {
        t = {{1000, 1001, 999}, {1000, 1, 999}, {2147483647, 2147483647, 200}, {2147483647, 1, 1}};
        CHECK(format("c", 'A', p - 2, t) == restated("c", 'A', p - 2, t));
    }
    t = {{5, 6}, {5, 1}, {7, 8}, {1, 8}};
    CHECK(format(long_name, 'C', bmk::MAX_LENGTH - 2, t) == restated(long_name, 'C', bmk::MAX_LENGTH - 2, t));
    t = {};
    for (int m = 0; m <= 100; ++m) {
        t.cp.push_back(100);
        t.mp.push_back(m);
        t.cm.push_back(m == 0 ? 0 : 2147483647);
        t.mm.push_back(int32_t(int64_t(m) * 2147483647 / 100));
    }
    CHECK(format("chrT", 'C', 0, t) == restated("chrT", 'C', 0, t));
    // a sum outside 0 <= mod <= cov is refused with its index
    {
        bmk::Name name;
        bmk::set_name(name, "chr1");
        for (const auto& cm : std::vector<std::pair<int32_t, int32_t>>{{5, 6}, {-1, 0}, {5, -1}}) {
            Tables u = {{1, 2, cm.first}, {1, 1, cm.second}, {0, 0, 0}, {0, 0, 0}};
            auto cp = exact(u.cp), mp = exact(u.mp), cmm = exact(u.cm), mm = exact(u.mm);
            int64_t lines = 0, bad = -1;
            CHECK(bmk::format_tables(name, 'C', 0, 3, cp.get(), mp.get(), cmm.get(), mm.get(), nullptr, 0, &lines, &bad) == -1 && bad == 2);
        }
    }
    // random tables against the restatement, and parsed back: the formatter's own text is inside the grammar
    std::mt19937_64 rng(11);
    for (int round = 0; round < 300; ++round) {
        const size_t n = size_t(rng() % 50);
        Tables u;
        for (size_t i = 0; i < n; ++i)
            for (int s = 0; s < 2; ++s) {
                const int32_t cv = int32_t(rng() % (round % 5 == 0 ? 2147483648ull : (round % 3 == 0 ? 3000 : 60)));
                const int32_t md = (cv && rng() % 3) ? int32_t(rng() % (uint64_t(cv) + 1)) : 0;
                (s ? u.cm : u.cp).push_back(cv);
                (s ? u.mm : u.mp).push_back(md);
            }
        const std::string chrom = round % 3 ? "chr" + std::to_string(round % 23) : std::string(size_t(1 + round % 60), 'k');
        const int64_t first = int64_t(rng() % uint64_t(bmk::MAX_LENGTH - int64_t(n)));
        const std::string text = format(chrom, 'C', first, u);
        CHECK(text == restated(chrom, 'C', first, u));
        r = parse(text, chrom.c_str());
        CHECK(r.bad == 0 && r.rows == std::count(text.begin(), text.end(), '\n'));
        size_t k = 0;
        for (size_t i = 0; i < n; ++i)
            for (int s = 0; s < 2; ++s)
                if ((s ? u.mm : u.mp)[i] > 0) {
                    CHECK(k < size_t(r.rows) && r.pos[k] == first + int64_t(i) && r.strand[k] == s && r.cov[k] == (s ? u.cm : u.cp)[i] && r.mod[k] == (s ? u.mm : u.mp)[i]);
                    ++k;
                }
        CHECK(k == size_t(r.rows));
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("MERGE-ASAN-OK\n");
    return 0;
}
