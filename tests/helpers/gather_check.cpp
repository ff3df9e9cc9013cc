// host/gather.hpp against a restatement that shares nothing with it (printf into a stream, the sum from a separate loop), on
// seeded random picks of every small size and on the shapes a gather file has (no pick -- an empty file --, ids and counts next
// to 2^32, depth sums beyond 32 bits), with and without the depth field -- built under AddressSanitizer + UBSan by
// tests/test_gather_abi.py.  Prints "ok <cases>"; with an argument, the file and the summary line of one fixed input, which the
// test compares with tests/gather_ref.py's.
#include <cinttypes>
#include <cstdio>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "gather.hpp"

static bool same(const std::vector<mk_pick> &picks, bool with_depth, uint64_t queries, uint64_t cells, uint32_t min_new)
{
    std::ostringstream want;
    want << "kept";
    uint64_t explained = 0;
    for (const mk_pick &x : picks) {
        char line[200];
        if (with_depth) snprintf(line, sizeof line, "%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu64 "\n", x.genome, x.fresh, x.covered, x.sketch_size, x.depth_sum);
        else snprintf(line, sizeof line, "%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32 "\n", x.genome, x.fresh, x.covered, x.sketch_size);
        want << line;
    }
    for (const mk_pick &x : picks) explained += x.fresh;
    std::string text = "kept";
    const uint64_t got = mkhost::format_gather(picks.data(), picks.size(), with_depth, text);
    if (text != want.str() || got != explained) { printf("differs at n = %zu\n", picks.size()); return false; }
    char line[400];
    snprintf(line, sizeof line, "gather: %" PRIu64 " queries, %" PRIu64 " of %" PRIu64 " seen cells explained by %zu genomes, each at least %" PRIu32 " new",
             queries, explained, cells, picks.size(), min_new);
    if (mkhost::gather_summary(queries, explained, cells, picks.size(), min_new) != line) { printf("summary differs at n = %zu\n", picks.size()); return false; }
    return true;
}

int main(int argc, char **)
{
    static_assert(sizeof(mk_pick) == 24, "mk_pick is 24 bytes");
    if (argc > 1) {
        const std::vector<mk_pick> picks{{7, 30, 41, 500, 95}, {1003, 30, 30, 480, 1ull << 40}, {0, 1, 4294967295u, 4294967295u, 0}};
        for (int with_depth = 0; with_depth < 2; ++with_depth) {
            std::string text;
            const uint64_t explained = mkhost::format_gather(picks.data(), picks.size(), with_depth != 0, text);
            printf("%s%s\n", text.c_str(), mkhost::gather_summary(620, explained, 99, picks.size(), 10).c_str());
        }
        return 0;
    }
    std::mt19937_64 rng(20266);
    unsigned cases = 0;
    for (uint32_t n = 0; n <= 70; ++n)                                     // (n = 0: no pick, the pointer of an empty vector)
        for (int rep = 0; rep < 20; ++rep, ++cases) {
            std::vector<mk_pick> picks(n);
            uint32_t fresh = 1 + (uint32_t)(rng() % 140000);
            for (uint32_t j = 0; j < n; ++j) {
                fresh = 1 + (uint32_t)(rng() % fresh);                     // never increasing
                picks[j].genome = (uint32_t)rng();
                picks[j].fresh = fresh;
                picks[j].covered = fresh + (uint32_t)(rng() % 1000);
                picks[j].sketch_size = picks[j].covered + (uint32_t)(rng() % 1000);
                picks[j].depth_sum = rep % 2 ? fresh + rng() % ((uint64_t)fresh * 254 + 1) : 0;
            }
            if (!same(picks, rep % 2 != 0, rng() % 100000, rng() >> (rng() % 64), 1 + (uint32_t)(rng() % 50))) return 1;
        }
    for (uint32_t n : {1u, 304u, 5000u}) {
        std::vector<mk_pick> picks(n, mk_pick{4294967295u, 131072, 131072, 131072, 255ull * 131072});
        if (!same(picks, false, 3ull * n, (uint64_t)1 << 25, 10) || !same(picks, true, 3ull * n, (uint64_t)1 << 25, 10)) return 1;
        cases += 2;
    }
    {   // the largest values there are: 2^28 partitions, counts and ids at the top of 32 bits, sums beyond them
        const std::vector<mk_pick> picks{{UINT32_MAX, UINT32_MAX, UINT32_MAX, UINT32_MAX, UINT64_MAX}, {0, 1u << 28, 1u << 28, UINT32_MAX, 255ull << 28}, {1, 1, 1, 1, 0}};
        if (!same(picks, true, UINT64_MAX, (uint64_t)1 << 44, UINT32_MAX) || !same(picks, false, 0, 0, 1)) return 1;
        cases += 2;
    }
    printf("ok %u\n", cases);
    return 0;
}
