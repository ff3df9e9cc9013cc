// host/cover.hpp against a restatement that shares nothing with it (printf into a stream, the count from a separate loop), on
// seeded random counts of every small size and on the shapes a cover file has (nothing covered, everything covered, the largest
// values) -- built under AddressSanitizer + UBSan by tests/test_cover_abi.py.  Prints "ok <cases>".
#include <cinttypes>
#include <cstdio>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "cover.hpp"

static bool same(const std::vector<uint32_t> &cov, const std::vector<uint32_t> &ss, uint64_t queries, uint64_t cells, uint32_t h, uint32_t fp_bits)
{
    std::ostringstream want;
    want << "kept";
    uint64_t genomes = 0;
    for (size_t j = 0; j < cov.size(); ++j) {
        if (cov[j] == 0) continue;
        char line[96];
        snprintf(line, sizeof line, "%zu\t%" PRIu32 "\t%" PRIu32 "\n", j, cov[j], ss[j]);
        want << line;
    }
    for (uint32_t x : cov) genomes += x != 0;
    std::string text = "kept";
    const uint64_t got = mkhost::format_cover(cov.data(), ss.data(), cov.size(), text);
    if (text != want.str() || got != genomes) { printf("differs at n = %zu\n", cov.size()); return false; }
    char line[256];
    snprintf(line, sizeof line, "cover: %" PRIu64 " queries, %" PRIu64 " of %" PRIu64 " cells seen, %" PRIu64 " genomes covered", queries, cells,
             (uint64_t)1 << (h + fp_bits), genomes);
    if (mkhost::cover_summary(queries, cells, h, fp_bits, genomes) != line) { printf("summary differs at n = %zu\n", cov.size()); return false; }
    return true;
}

int main()
{
    std::mt19937_64 rng(20262);
    unsigned cases = 0;
    for (uint32_t n = 0; n <= 70; ++n)
        for (int rep = 0; rep < 20; ++rep, ++cases) {
            std::vector<uint32_t> cov(n), ss(n);
            for (uint32_t j = 0; j < n; ++j) {
                ss[j] = (uint32_t)(rng() % 140000);
                cov[j] = rng() % 3 && ss[j] ? (uint32_t)(rng() % (ss[j] + 1)) : 0;
            }
            const uint32_t h = 1 + (uint32_t)(rng() % 28), bits = rng() % 2 ? 8 : 16;
            if (!same(cov, ss, rng() % 100000, rng() % ((uint64_t)1 << (h + bits)), h, bits)) return 1;
        }
    for (uint32_t n : {1u, 304u, 5000u}) {
        std::vector<uint32_t> none(n, 0), all(n, 131072), ss(n, 131072);
        if (!same(none, ss, 0, 0, 17, 8) || !same(all, ss, 3ull * n, (uint64_t)1 << 25, 17, 8)) return 1;
        cases += 2;
    }
    {   // the largest values there are: 2^28 partitions of 16-bit fingerprints, counts at the top of 32 bits
        std::vector<uint32_t> cov{UINT32_MAX, 0, 1u << 28}, ss{UINT32_MAX, UINT32_MAX, 1u << 28};
        if (!same(cov, ss, UINT64_MAX, (uint64_t)1 << 44, 28, 16)) return 1;
        ++cases;
    }
    printf("ok %u\n", cases);
    return 0;
}
