// TEST INFRASTRUCTURE - not part of the product.  dm_cluster_bed_format (deepmod_amd/csrc/bedtext.inc: the lines of detect --clusterCpG) under
// -fsanitize=address,undefined, as a program: tests/asan/host_shim.cpp (the host part of the C ABI, compiled by g++) is included as it is, and
// every column and the text live in heap blocks of exactly their size, so that a read or a write one element outside them is a sanitizer report.
// Zero sites, one site, cov > 1000, the longest values the formatter accepts, random records against a plain restatement, refused records.
// tests/test_cluster_fused.py builds and runs it.
#include "asan/host_shim.cpp"

#include <cinttypes>
#include <cstdlib>
#include <memory>
#include <random>

namespace {

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {       // a block of exactly v.size() elements (new T[0] is a valid, unreadable block)
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

struct Rec {
    int64_t pos;
    int32_t cov, mod, nw;
};

// sum_chr_mod.py:63's row + " <new>\n" (hm_cluster_predict.py:170)
std::string restated(const std::string& chrom, char strand, char base, const std::vector<Rec>& recs) {
    std::string out;
    char buf[512];
    for (const Rec& r : recs) {
        std::snprintf(buf, sizeof buf, "%s %" PRId64 " %" PRId64 " %c %d %c  %" PRId64 " %" PRId64 " 0,0,0 %d %" PRId64 " %d %d\n", chrom.c_str(), r.pos, r.pos + 1, base,
                      r.cov < 1000 ? r.cov : 1000, strand, r.pos, r.pos + 1, r.cov, r.cov > 0 ? int64_t(r.mod) * 100 / r.cov : int64_t(0), r.mod, r.nw);
        out += buf;
    }
    return out;
}

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

// formats into a block of exactly the bound the sizing call returned; rc < 0: the error code
int64_t run(const std::string& chrom, char strand, const std::vector<Rec>& recs, std::string* text) {
    std::vector<int64_t> pos;
    std::vector<int32_t> cov, mod, nw;
    for (const Rec& r : recs) {
        pos.push_back(r.pos);
        cov.push_back(r.cov);
        mod.push_back(r.mod);
        nw.push_back(r.nw);
    }
    auto p = exact(pos);
    auto c = exact(cov), m = exact(mod), w = exact(nw);
    const int64_t n = int64_t(recs.size());
    const int64_t bound = dm_cluster_bed_format(chrom.c_str(), strand, 'C', p.get(), c.get(), m.get(), w.get(), n, nullptr, 0);
    if (bound < 0) return bound;
    CHECK(bound == n * int64_t(chrom.size() + 128));
    std::unique_ptr<char[]> small(new char[1]);               // a capacity below the bound: nothing is written, the bound comes back
    small[0] = '#';
    CHECK(dm_cluster_bed_format(chrom.c_str(), strand, 'C', p.get(), c.get(), m.get(), w.get(), n, small.get(), bound - 1) == bound || bound == 0);
    CHECK(small[0] == '#');
    std::unique_ptr<char[]> out(new char[size_t(bound)]);
    const int64_t got = dm_cluster_bed_format(chrom.c_str(), strand, 'C', p.get(), c.get(), m.get(), w.get(), n, out.get(), bound);
    CHECK(got >= 0 && got <= bound);
    if (got >= 0) text->assign(out.get(), out.get() + got);
    return got;
}

}  // namespace

int main() {
    std::string text;
    // zero sites: no byte, also with null columns
    CHECK(run("chr1", '+', {}, &text) == 0 && text.empty());
    CHECK(dm_cluster_bed_format("chr1", '+', 'C', nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0) == 0);
    // one site
    CHECK(run("chr1", '+', {{10468, 7, 3, 61}}, &text) > 0);
    CHECK(text == "chr1 10468 10469 C 7 +  10468 10469 0,0,0 7 42 3 61\n");
    // cov > 1000: column 5 is capped, column 10 is not
    CHECK(run("chrX", '-', {{5, 1500, 700, 0}, {6, 1000, 1000, 100}, {9, 999, 1, 99}}, &text) > 0);
    CHECK(text == "chrX 5 6 C 1000 -  5 6 0,0,0 1500 46 700 0\nchrX 6 7 C 1000 -  6 7 0,0,0 1000 100 1000 100\nchrX 9 10 C 999 -  9 10 0,0,0 999 0 1 99\n");
    // the longest line the formatter accepts fits the bound of its contig name: 13-digit positions, ten-digit counts, mod far above cov
    const std::vector<Rec> longest = {{(int64_t(1) << 40) - 1, 2147483647, 2147483647, 2147483647}, {(int64_t(1) << 40) - 1, 1, 2147483647, 2147483647}};
    CHECK(run("", '+', longest, &text) > 0 && text == restated("", '+', 'C', longest));
    CHECK(run("c", '+', longest, &text) > 0 && text == restated("c", '+', 'C', longest));
    // refused records: an error code, nothing read beyond the columns
    CHECK(run("chr1", '+', {{-1, 1, 1, 1}}, &text) == DM_EINVAL);
    CHECK(run("chr1", '+', {{int64_t(1) << 40, 1, 1, 1}}, &text) == DM_EINVAL);
    CHECK(run("chr1", '+', {{1, -1, 1, 1}}, &text) == DM_EINVAL);
    CHECK(run("chr1", '+', {{1, 1, -1, 1}}, &text) == DM_EINVAL);
    CHECK(run("chr1", '+', {{1, 1, 1, -1}}, &text) == DM_EINVAL);
    CHECK(dm_cluster_bed_format(nullptr, '+', 'C', nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0) == DM_EINVAL);
    CHECK(dm_cluster_bed_format("chr1", '+', 'C', nullptr, nullptr, nullptr, nullptr, 1, nullptr, 0) == DM_EINVAL);
    CHECK(dm_cluster_bed_format("chr1", '+', 'C', nullptr, nullptr, nullptr, nullptr, -1, nullptr, 0) == DM_EINVAL);
    // random records against the restatement
    std::mt19937_64 rng(7);
    for (int round = 0; round < 200; ++round) {
        std::vector<Rec> recs(rng() % 40);
        for (Rec& r : recs) {
            r.cov = int32_t(rng() % (round % 4 == 0 ? 5000 : 60));
            r.mod = r.cov ? int32_t(rng() % (uint64_t(r.cov) + 1)) : 0;
            r.pos = int64_t(rng() % (round % 7 == 0 ? (uint64_t(1) << 40) : 300000000ull));
            r.nw = int32_t(rng() % 101);
        }
        const std::string chrom = round % 3 ? "chr" + std::to_string(round % 23) : std::string(size_t(round % 50), 'k');
        const char strand = round % 2 ? '+' : '-';
        CHECK(run(chrom, strand, recs, &text) >= 0);
        CHECK(text == restated(chrom, strand, 'C', recs));
    }
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("CLUSTER-ASAN-OK\n");
    return 0;
}
