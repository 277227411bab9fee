// TEST INFRASTRUCTURE - not part of the product.  The line routine of `siteperf` (deepmod_amd/csrc/siteperf.inc: spk::parse_line / parse_text on the
// field routines of bedline.inc - the code sp_parse_kernel of siteperf.hip.inc runs) under -fsanitize=address,undefined, as a program.  Every text and
// every record array lives in a heap block of exactly its size, so that a read or a write one byte outside it is a sanitizer report.  The good and
// the bad lines of tests/test_siteperf_host.py, texts cut at every byte (a truncated last line, a missing final '\n'), and random byte mutations of
// all of them: whatever the bytes, a line that is accepted gives a record the kernels can index with - a position on the contig, a percentage
// <= 100, modified <= coverage, a strand of 0 or 1.  tests/test_siteperf_host.py builds and runs it.
#include "../deepmod_amd/csrc/siteperf.inc"

#include <algorithm>
#include <cstdio>
#include <memory>
#include <random>
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
    int64_t rows = 0, bad = 0;
    std::vector<int32_t> pos, cov, pct, mod;
    std::vector<uint8_t> strand, base;
};

std::string replaced(std::string s, const std::string& from, const std::string& to) {       // Python's bytes.replace
    for (size_t at = 0; (at = s.find(from, at)) != std::string::npos; at += to.size()) s.replace(at, from.size(), to);
    return s;
}

// the text in a block of exactly its size; the records in blocks of exactly `rows` elements (sized by a first call with cap 0)
Parsed parse(const std::string& text, const char* contig, long long contig_len) {
    bed::Name name;
    CHECK(bed::set_name(name, contig));
    std::unique_ptr<char[]> t(new char[text.size()]);
    std::copy(text.begin(), text.end(), t.get());
    Parsed r;
    r.rows = spk::parse_text(t.get(), int64_t(text.size()), name, contig_len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &r.bad);
    const size_t n = size_t(r.rows);
    std::unique_ptr<int32_t[]> pos(new int32_t[n]), cov(new int32_t[n]), pct(new int32_t[n]), mod(new int32_t[n]);
    std::unique_ptr<uint8_t[]> strand(new uint8_t[n]), base(new uint8_t[n]);
    int64_t bad2 = -1;
    CHECK(spk::parse_text(t.get(), int64_t(text.size()), name, contig_len, pos.get(), strand.get(), base.get(), cov.get(), pct.get(), mod.get(), r.rows, &bad2) == r.rows &&
          bad2 == r.bad);
    r.pos.assign(pos.get(), pos.get() + n);
    r.cov.assign(cov.get(), cov.get() + n);
    r.pct.assign(pct.get(), pct.get() + n);
    r.mod.assign(mod.get(), mod.get() + n);
    r.strand.assign(strand.get(), strand.get() + n);
    r.base.assign(base.get(), base.get() + n);
    const int64_t want_rows = std::count(text.begin(), text.end(), '\n') + ((!text.empty() && text.back() != '\n') ? 1 : 0);
    CHECK(r.rows == want_rows && r.bad >= 0 && r.bad <= r.rows);
    // what the kernels index with: every record, of an accepted line (and the zeros of a refused one), is inside the contig and the histogram
    for (size_t k = 0; k < n; ++k)
        CHECK(r.pos[k] >= 0 && r.pos[k] < contig_len && r.pct[k] >= 0 && r.pct[k] <= 100 && r.mod[k] >= 0 && r.mod[k] <= r.cov[k] && r.strand[k] <= 1);
    return r;
}

}  // namespace

int main() {
    const std::string good = "c1\t5\t6\tC\t7\t+\t5\t6\t0,0,0\t7\t42\t3\n";
    const std::string spaced = replaced(replaced(good, "\t", " "), "+", "-");
    Parsed r = parse(good + spaced, "c1", 10);
    CHECK(r.rows == 2 && r.bad == 0);
    CHECK(r.pos == (std::vector<int32_t>{5, 5}) && r.strand == (std::vector<uint8_t>{0, 1}) && r.base == (std::vector<uint8_t>{67, 67}) &&
          r.cov == (std::vector<int32_t>{7, 7}) && r.pct == (std::vector<int32_t>{42, 42}) && r.mod == (std::vector<int32_t>{3, 3}));
    // the largest numbers, a thirteenth field, no final newline
    std::string wide = replaced(good, "\t7\t42\t3", "\t2147483647\t42\t2147483647");
    wide.pop_back();
    wide += "\textra field";
    r = parse(wide, "c1", 10);
    CHECK(r.rows == 1 && r.bad == 0 && r.cov[0] == 2147483647 && r.mod[0] == 2147483647);
    // every violation, as line 2 of three and as a last line without its '\n'
    std::string eleven = good.substr(0, good.rfind('\t')) + "\n";
    const std::vector<std::string> bad_lines = {
        replaced(good, "\n", "\r\n"), "\n", replaced(good, "\tC\t", "\t\tC\t"), replaced(good, "c1", "c2"), replaced(good, "\t42\t", "\t+42\t"),
        replaced(good, "\t42\t", "\t101\t"), replaced(good, "\t5\t6\tC", "\t10\t11\tC"), replaced(good, "\t7\t42\t3", "\t2\t42\t3"), replaced(good, "\t+\t", "\t*\t"),
        replaced(good, "\tC\t", "\tCC\t"), eleven, replaced(good, "\t7\t42", "\t12345678901\t42"), replaced(good, "\t7\t42", "\t2147483648\t42"),
        replaced(good, "3\n", "3\t\n"), "\t" + good, replaced(good, "c1", "c11"), replaced(good, "c1", "c"), replaced(good, "\t3\n", "\t3\x01\n"),
        replaced(good, "\t3\n", "\t3\x7f\n"), replaced(good, "\t3\n", "\t\n")};
    for (const std::string& line : bad_lines) {
        r = parse(good + line + good, "c1", 10);
        CHECK(r.rows == 3 && r.bad == 2);
        CHECK(r.pos[1] == 0 && r.cov[1] == 0 && r.pct[1] == 0 && r.mod[1] == 0 && r.strand[1] == 0 && r.base[1] == 0 && r.pos[2] == 5);
        if (line != "\n") {
            r = parse(good + line.substr(0, line.size() - 1), "c1", 10);
            CHECK(r.rows == 2 && r.bad == 2);
        }
    }
    r = parse(good.substr(0, good.size() - 1) + std::string(1, '\0') + "\n", "c1", 10);                      // a NUL byte
    CHECK(r.rows == 1 && r.bad == 1);
    CHECK(parse("", "c1", 10).rows == 0);
    bed::Name nm;
    CHECK(!bed::set_name(nm, "") && !bed::set_name(nm, nullptr) && !bed::set_name(nm, std::string(256, 'k').c_str()) && bed::set_name(nm, std::string(255, 'k').c_str()) &&
          nm.n == 255);
    const std::string long_name(255, 'q');
    r = parse(long_name + good.substr(2) + long_name.substr(1) + good.substr(2), long_name.c_str(), 10);
    CHECK(r.rows == 2 && r.bad == 2 && r.pos[0] == 5);
    // a text cut at every byte: nothing behind the cut is read.  The numbers of these lines are in range from their first digit on, so the verdict
    // on a cut last line is that of a plain restatement: twelve or more fields, none of them empty
    const std::string whole = good + spaced + wide;
    for (size_t cut = 0; cut <= whole.size(); ++cut) {
        const std::string text = whole.substr(0, cut);
        r = parse(text, "c1", 10);
        bool last_ok = true;
        if (!text.empty() && text.back() != '\n') {
            const size_t nl = text.rfind('\n');
            const std::string line = text.substr(nl == std::string::npos ? 0 : nl + 1);
            size_t fields = 1;
            for (size_t k = 0; k < line.size(); ++k)
                if (line[k] == ' ' || line[k] == '\t') {
                    ++fields;
                    last_ok = last_ok && k > 0 && k + 1 < line.size() && line[k + 1] != ' ' && line[k + 1] != '\t';
                }
            last_ok = last_ok && fields >= 12;
        }
        CHECK(r.bad == (last_ok ? 0 : r.rows));
    }
    // random byte mutations of the good and the bad lines: whatever comes out is checked by parse() itself
    std::mt19937_64 rng(7);
    std::vector<std::string> pool = bad_lines;
    for (int k = 0; k < 8; ++k) pool.insert(pool.end(), {good, spaced, wide + "\n"});
    const char bytes[] = "\t \n\r0123456789+-C,c1\x00\x01\x7f\xff";
    int64_t accepted = 0, refused = 0;
    for (int round = 0; round < 60000; ++round) {
        std::string text = good + pool[size_t(rng() % pool.size())] + pool[size_t(rng() % pool.size())];
        for (int k = int(rng() % 3); k >= 0; --k) {
            const size_t at = size_t(rng() % text.size());
            const char c = round % 4 ? bytes[rng() % (sizeof bytes - 1)] : char(rng() & 0xff);
            switch (rng() % 3) {
            case 0: text[at] = c; break;
            case 1: text.insert(at, 1, c); break;
            default: text.erase(at, 1);
            }
        }
        r = parse(text, "c1", 1 + (long long)(rng() % 12));
        (r.bad ? refused : accepted) += 1;
    }
    CHECK(accepted > 1000 && refused > 1000);                       // (both sides of the grammar were reached)
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("SITEPERF-ASAN-OK\n");
    return 0;
}
