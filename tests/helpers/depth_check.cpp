// host/depth.hpp against a restatement that shares nothing with it (printf into a stream, the count from a separate loop), on
// seeded random results of every small size and on the shapes a depth file has (empty input, nothing covered -- no line --,
// everything covered, sums beyond 32 bits, ids and counts next to 2^32) -- built under AddressSanitizer + UBSan by
// tests/test_depth_abi.py.  Prints "ok <cases>".
#include <cinttypes>
#include <cstdio>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "depth.hpp"

static bool same(const std::vector<mk_depth> &d, const std::vector<uint32_t> &ss, uint64_t queries, uint64_t cells, uint64_t saturated, uint32_t h,
                 uint32_t fp_bits)
{
    std::ostringstream want;
    want << "kept";
    uint64_t genomes = 0;
    for (size_t j = 0; j < d.size(); ++j) {
        if (d[j].covered == 0) continue;
        char line[160];
        snprintf(line, sizeof line, "%zu\t%" PRIu32 "\t%" PRIu64 "\t%" PRIu32 "\t%" PRIu32 "\n", j, d[j].median, d[j].sum, d[j].covered, ss[j]);
        want << line;
    }
    for (const mk_depth &x : d) genomes += x.covered != 0;
    std::string text = "kept";
    const uint64_t got = mkhost::format_depth(d.data(), ss.data(), d.size(), text);
    if (text != want.str() || got != genomes) { printf("differs at n = %zu\n", d.size()); return false; }
    char line[320];
    snprintf(line, sizeof line, "depth: %" PRIu64 " queries, %" PRIu64 " of %" PRIu64 " cells seen, %" PRIu64 " at 255, %" PRIu64 " genomes covered",
             queries, cells, (uint64_t)1 << (h + fp_bits), saturated, genomes);
    if (mkhost::depth_summary(queries, cells, saturated, h, fp_bits, genomes) != line) { printf("summary differs at n = %zu\n", d.size()); return false; }
    return true;
}

int main()
{
    static_assert(sizeof(mk_depth) == 16, "mk_depth is 16 bytes");
    std::mt19937_64 rng(20265);
    unsigned cases = 0;
    for (uint32_t n = 0; n <= 70; ++n)                                     // (n = 0: empty input, the pointers of empty vectors)
        for (int rep = 0; rep < 20; ++rep, ++cases) {
            std::vector<mk_depth> d(n);
            std::vector<uint32_t> ss(n);
            for (uint32_t j = 0; j < n; ++j) {
                ss[j] = (uint32_t)(rng() % 140000);
                d[j].covered = rng() % 3 && ss[j] ? (uint32_t)(rng() % (ss[j] + 1)) : 0;
                d[j].median = d[j].covered ? 1 + (uint32_t)(rng() % 255) : 0;
                d[j].sum = d[j].covered ? d[j].covered + rng() % ((uint64_t)d[j].covered * 254 + 1) : 0;
            }
            const uint32_t h = 1 + (uint32_t)(rng() % 28), bits = rng() % 2 ? 8 : 16;
            const uint64_t all = (uint64_t)1 << (h + bits), cells = rng() % all;
            if (!same(d, ss, rng() % 100000, cells, cells ? rng() % cells : 0, h, bits)) return 1;
        }
    for (uint32_t n : {1u, 304u, 5000u}) {
        std::vector<mk_depth> none(n, mk_depth{0, 0, 0}), all(n, mk_depth{255ull * 131072, 131072, 255});
        std::vector<uint32_t> ss(n, 131072);
        // (a line is skipped by covered alone: a sum or a median beside covered = 0 changes nothing)
        none[n / 2].sum = 77;
        none[n / 2].median = 3;
        if (!same(none, ss, 0, 0, 0, 17, 8) || !same(all, ss, 3ull * n, (uint64_t)1 << 25, (uint64_t)1 << 25, 17, 8)) return 1;
        cases += 2;
    }
    {   // the largest values there are: 2^28 partitions of 16-bit fingerprints, counts at the top of 32 bits, sums beyond them
        std::vector<mk_depth> d{{255ull * UINT32_MAX, UINT32_MAX, 255}, {0, 0, 0}, {(1ull << 32) + 1, 1u << 28, 16}, {UINT64_MAX, UINT32_MAX - 1, UINT32_MAX}};
        std::vector<uint32_t> ss{UINT32_MAX, UINT32_MAX, 1u << 28, UINT32_MAX};
        if (!same(d, ss, UINT64_MAX, (uint64_t)1 << 44, ((uint64_t)1 << 44) - 1, 28, 16)) return 1;
        ++cases;
    }
    printf("ok %u\n", cases);
    return 0;
}
