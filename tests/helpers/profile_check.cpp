// host/profile.hpp against a restatement that shares nothing with it (printf into a stream, counts from separate loops), on
// seeded random counters of every small size, on the shapes a profile has (nothing listed, everything listed, counters
// beyond 32 bits) -- built under AddressSanitizer + UBSan by tests/test_tally_abi.py.  Prints "ok <cases>".
#include <cinttypes>
#include <cstdio>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "profile.hpp"

static bool same(const std::vector<mk_tally> &t, uint64_t queries)
{
    std::ostringstream want;
    want << "kept";
    uint64_t assigned = 0, unique = 0, genomes = 0;
    for (size_t j = 0; j < t.size(); ++j) {
        if (t[j].listed == 0) continue;
        char line[128];
        snprintf(line, sizeof line, "%zu\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\n", j, t[j].best, t[j].unique, t[j].listed, t[j].best_matches);
        want << line;
    }
    for (const mk_tally &x : t) assigned += x.listed ? x.best : 0;
    for (const mk_tally &x : t) unique += x.listed ? x.unique : 0;
    for (const mk_tally &x : t) genomes += x.listed != 0;
    std::string text = "kept";
    mkhost::ProfileCounts c;
    c.assigned = c.unique = c.genomes = 77;                      // (the writer starts from zero, whatever it is handed)
    mkhost::format_profile(t.data(), t.size(), text, c);
    if (text != want.str() || c.assigned != assigned || c.unique != unique || c.genomes != genomes) { printf("differs at n = %zu\n", t.size()); return false; }
    char line[256];
    snprintf(line, sizeof line, "profile: %" PRIu64 " queries, %" PRIu64 " assigned, %" PRIu64 " listing one genome only, %" PRIu64 " genomes listed",
             queries, assigned, unique, genomes);
    if (mkhost::profile_summary(queries, c) != line) { printf("summary differs at n = %zu\n", t.size()); return false; }
    return true;
}

int main()
{
    static_assert(sizeof(mk_tally) == 32, "four 64-bit counters");
    std::mt19937_64 rng(20261);
    unsigned cases = 0;
    for (uint32_t n = 0; n <= 70; ++n)
        for (int rep = 0; rep < 20; ++rep, ++cases) {
            // a genome is listed by some queries or by none; unique and best are among the listed
            std::vector<mk_tally> t(n);
            for (mk_tally &x : t) {
                x.listed = rng() % 3 ? rng() % 1000 : 0;
                x.unique = x.listed ? rng() % (x.listed + 1) : 0;
                x.best = x.listed ? rng() % (x.listed + 1) : 0;
                x.best_matches = x.best * (rng() % 4096);
            }
            if (!same(t, rng() % 100000)) return 1;
        }
    for (uint32_t n : {1u, 304u, 5000u}) {
        std::vector<mk_tally> none(n, mk_tally{0, 0, 0, 0}), all(n, mk_tally{3, 1, 2, 900});
        if (!same(none, 0) || !same(all, 3ull * n)) return 1;
        cases += 2;
    }
    {   // counters beyond 32 bits, and the largest there are
        std::vector<mk_tally> t(3, mk_tally{1ull << 40, 1ull << 33, 1ull << 39, 1ull << 52});
        t[1] = mk_tally{UINT64_MAX, 0, UINT64_MAX, UINT64_MAX};
        if (!same(t, 1ull << 41)) return 1;
        ++cases;
    }
    printf("ok %u\n", cases);
    return 0;
}
