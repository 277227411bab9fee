// TEST INFRASTRUCTURE - not part of the product.  The class rule and the line routine of `bslabels` (deepmod_amd/csrc/bslabels.inc: blk::class_of,
// emit_position, format_classes, the code the kernels of bslabels.hip.inc run) under -fsanitize=address,undefined, as a program.  Every class array
// and every text lives in a heap block of exactly its size, so that a read or a write one byte outside it is a sanitizer report.  The text against
// snprintf at every digit count of a position (1 to 10), names of 1 and 63 bytes, a missing strand, a capacity one byte short; the class against a
// plain restatement of the rules over every combination of two replicates' slots at the edges.  tests/test_bslabels_host.py builds and runs it.
#include "../deepmod_amd/csrc/bslabels.inc"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
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

std::string expected(const std::string& name, int list, int64_t first, const std::vector<uint8_t>& p, const std::vector<uint8_t>& m, bool has_p, bool has_m) {
    std::string out;
    char buf[128];
    const size_t n = has_p ? p.size() : m.size();
    for (size_t i = 0; i < n; ++i)
        for (int s = 0; s < 2; ++s) {
            if ((s == 0 && (!has_p || p[i] != list)) || (s == 1 && (!has_m || m[i] != list))) continue;
            std::snprintf(buf, sizeof buf, "%s %c %lld\n", name.c_str(), s ? '-' : '+', (long long)(first + int64_t(i)));
            out += buf;
        }
    return out;
}

// the class arrays and the output in heap blocks of exactly their sizes
void format_case(const std::string& name, int64_t first, const std::vector<uint8_t>& p, const std::vector<uint8_t>& m, bool has_p, bool has_m) {
    blk::Name nm = {};
    CHECK(blk::set_name(nm, name.c_str()));
    const size_t n = has_p ? p.size() : m.size();
    std::unique_ptr<uint8_t[]> bp(has_p ? new uint8_t[n] : nullptr), bm(has_m ? new uint8_t[n] : nullptr);
    if (has_p) std::copy(p.begin(), p.end(), bp.get());
    if (has_m) std::copy(m.begin(), m.end(), bm.get());
    for (int list = blk::C_FUL; list <= blk::C_NO; ++list) {
        const std::string want = expected(name, list, first, p, m, has_p, has_m);
        int64_t lines = -1;
        const int64_t bytes = blk::format_classes(nm, list, first, int64_t(n), bp.get(), bm.get(), nullptr, 0, &lines);
        CHECK(bytes == int64_t(want.size()) && lines == int64_t(std::count(want.begin(), want.end(), '\n')));
        std::unique_ptr<char[]> out(new char[size_t(bytes)]);
        CHECK(blk::format_classes(nm, list, first, int64_t(n), bp.get(), bm.get(), out.get(), bytes, &lines) == bytes);
        CHECK(std::string(out.get(), size_t(bytes)) == want);
        if (bytes > 0) {                                             // one byte short: the size is returned and nothing is written
            std::unique_ptr<char[]> small(new char[size_t(bytes - 1)]);
            std::fill(small.get(), small.get() + bytes - 1, '\x5a');
            CHECK(blk::format_classes(nm, list, first, int64_t(n), bp.get(), bm.get(), small.get(), bytes - 1, &lines) == bytes);
            CHECK(std::all_of(small.get(), small.get() + bytes - 1, [](char c) { return c == '\x5a'; }));
        }
    }
}

int restated(const unsigned* slot, int R, int cov, int hi, int lo, bool site) {
    int have = 0, deep = 0, high = 0, low = 0;
    for (int r = 0; r < R; ++r) {
        if (!slot[r]) continue;
        ++have;
        deep += int(slot[r] & 0xffffu) >= cov;
        high += int((slot[r] >> 16) & 0x7fu) >= hi;
        low += int((slot[r] >> 16) & 0x7fu) <= lo;
    }
    if (!have) return blk::C_NONE;
    if (!site) return blk::C_OFF;
    if (have == R && deep == R && high == R) return blk::C_FUL;
    if (have == R && deep == R && low == R) return blk::C_NO;
    return blk::C_ANY;
}

}  // namespace

int main() {
    // positions at every digit count, both sides of every power of ten, the largest position
    const int64_t edges[] = {0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000, 2147483646};
    const std::vector<uint8_t> p = {1, 2, 3, 4, 0, 1, 1}, m = {3, 2, 1, 0, 4, 1, 2};
    for (const std::string& name : {std::string("c"), std::string(63, 'k'), std::string("chr10")})
        for (int64_t e : edges) {
            const int64_t first = std::min<int64_t>(e, blk::MAX_LENGTH - int64_t(p.size()));                 // the last position stays <= 2^31 - 2
            format_case(name, first, p, m, true, true);
            format_case(name, first, p, m, true, false);
            format_case(name, first, p, m, false, true);
            format_case(name, e, {1}, {1}, true, true);
        }
    format_case("chr1", 5, {}, {}, true, true);                                                                  // no position at all
    format_case("chr1", 5, {0, 4, 0}, {4, 0, 0}, true, true);                                                    // no line
    blk::Name nm = {};
    CHECK(!blk::set_name(nm, std::string(64, 'k').c_str()) && !blk::set_name(nm, "") && !blk::set_name(nm, "a b") && !blk::set_name(nm, nullptr));
    // the class of a key: 1 to 4 replicates, every slot one of the edge values, the slots `stride` apart in a block of exactly its size
    const int cov = 5, hi = 90, lo = 10;
    std::vector<unsigned> values = {0u};
    for (unsigned c : {4u, 5u, 65535u})
        for (unsigned pc : {0u, 10u, 11u, 89u, 90u, 100u}) values.push_back(blk::PRESENT | pc << 16 | c);
    for (int R = 1; R <= blk::MAX_REP; ++R) {
        const long long stride = 3;
        std::unique_ptr<unsigned[]> slots(new unsigned[size_t((R - 1) * stride + 1)]);
        std::vector<size_t> pick(size_t(R), 0);
        const size_t step = R >= 3 ? 3 : 1;                                                                       // (a third of the values at R >= 3)
        for (bool more = true; more;) {
            unsigned flat[blk::MAX_REP];
            for (int r = 0; r < R; ++r) flat[r] = slots[size_t(r * stride)] = values[pick[size_t(r)]];
            const blk::Rule rule = {R, cov, hi, lo};
            for (int site = 0; site < 2; ++site) CHECK(blk::class_of(slots.get(), stride, rule, site != 0) == restated(flat, R, cov, hi, lo, site != 0));
            int r = 0;
            for (; r < R; ++r) {
                pick[size_t(r)] += step;
                if (pick[size_t(r)] < values.size()) break;
                pick[size_t(r)] = 0;
            }
            more = r < R;
        }
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("BSLABELS-ASAN-OK\n");
    return 0;
}
