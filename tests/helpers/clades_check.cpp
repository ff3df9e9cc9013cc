// host/clades.hpp: the parser of -L's file on good files and on every refusal, the map it makes, and the writer of -p's file
// against a restatement that shares nothing with it (printf into a stream, counts from separate loops) on seeded random
// counters -- built under AddressSanitizer + UBSan by tests/test_clade_abi.py.  Prints "ok <cases>".
#include <cinttypes>
#include <cstdio>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "clades.hpp"

static unsigned cases = 0;

static bool fail(const char *what, const std::string &text)
{
    printf("%s: ", what);
    for (char ch : text) ch == '\n' ? printf("\\n") : ch == '\r' ? printf("\\r") : printf("%c", ch);
    printf("\n");
    return false;
}

// a good file: the clades it must give, as lists of ids
static bool good(const std::string &text, const std::vector<std::vector<uint32_t>> &want)
{
    ++cases;
    mkhost::CladeList l;
    std::string why = "kept";
    if (!mkhost::parse_clades(text, "f", l, why) || why != "kept") return fail("refused", text);
    std::vector<uint32_t> ids, clade, first, members;
    for (size_t c = 0; c < want.size(); ++c) {
        first.push_back(want[c].front());
        members.push_back((uint32_t)want[c].size());
        for (uint32_t g : want[c]) { ids.push_back(g); clade.push_back((uint32_t)c); }
    }
    if (l.ids != ids || l.clade != clade || l.first_id != first || l.members != members) return fail("parsed otherwise", text);
    // the map: named genomes carry their clade, every other is left out; an index one genome short refuses the last id
    if (ids.back() > 1000000u) return true;                      // (a map is an array of the index's size)
    const uint64_t G = (uint64_t)ids.back() + 3;
    std::vector<uint32_t> map;
    if (!mkhost::clade_map_of(l, G, map, why) || map.size() != G) return fail("no map", text);
    std::vector<uint32_t> expect(G, MK_NO_CLADE);
    for (size_t i = 0; i < ids.size(); ++i) expect[ids[i]] = clade[i];
    if (map != expect) return fail("map differs", text);
    if (!mkhost::clade_map_of(l, ids.back() + 1ull, map, why)) return fail("an index that just holds the ids was refused", text);
    if (mkhost::clade_map_of(l, ids.back(), map, why) || why.find("genome id " + std::to_string(ids.back()) + " is beyond") == std::string::npos)
        return fail("an id beyond the index was taken", text);
    return true;
}

// a refusal: the message names the line (or, for a file without ids, the file)
static bool bad(const std::string &text, const std::string &names)
{
    ++cases;
    mkhost::CladeList l;
    std::string why;
    if (mkhost::parse_clades(text, "the_file", l, why)) return fail("taken", text);
    if (why.rfind("-L: ", 0) != 0 || why.find(names) == std::string::npos || why.find("the_file") == std::string::npos) return fail(why.c_str(), text);
    return true;
}

static bool same(const std::vector<mk_clade_tally> &t, const std::vector<uint32_t> &first, const std::vector<uint32_t> &members, uint64_t queries)
{
    ++cases;
    std::ostringstream want;
    want << "kept";
    uint64_t assigned = 0, unique = 0, clades = 0;
    for (size_t c = 0; c < t.size(); ++c) {
        if (t[c].listed == 0) continue;
        char line[256];
        snprintf(line, sizeof line, "%zu\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\n", c, first[c], members[c],
                 t[c].best, t[c].unique, t[c].listed, t[c].best_matches, t[c].hits);
        want << line;
    }
    for (const mk_clade_tally &x : t) assigned += x.listed ? x.best : 0;
    for (const mk_clade_tally &x : t) unique += x.listed ? x.unique : 0;
    for (const mk_clade_tally &x : t) clades += x.listed != 0;
    std::string text = "kept";
    mkhost::CladeCounts c;
    c.assigned = c.unique = c.clades = 77;                       // (the writer starts from zero, whatever it is handed)
    mkhost::format_clade_profile(t.data(), first.data(), members.data(), t.size(), text, c);
    if (text != want.str() || c.assigned != assigned || c.unique != unique || c.clades != clades) { printf("differs at n = %zu\n", t.size()); return false; }
    char line[256];
    snprintf(line, sizeof line, "clades: %" PRIu64 " queries, %" PRIu64 " assigned, %" PRIu64 " listing one clade only, %" PRIu64 " clades listed",
             queries, assigned, unique, clades);
    if (mkhost::clade_summary(queries, c) != line) { printf("summary differs at n = %zu\n", t.size()); return false; }
    return true;
}

int main()
{
    static_assert(sizeof(mk_clade_tally) == 40, "five 64-bit counters");
    static_assert(MK_NO_CLADE == 0xffffffffu, "the left-out mark");
    // ---- the parser on good files: -F's own layout, one clade, no newline at the end, blank lines at either end and doubled,
    // CR LF, blanks around an id, the largest id there is
    if (!good("0\n1\n\n2\n", {{0, 1}, {2}})) return 1;
    if (!good("7\n", {{7}})) return 1;
    if (!good("7", {{7}})) return 1;
    if (!good("3\n5\n9", {{3, 5, 9}})) return 1;
    if (!good("0\n\n1\n\n2\n\n3\n", {{0}, {1}, {2}, {3}})) return 1;
    if (!good("\n\n4\n5\n\n\n\n8\n\n\n", {{4, 5}, {8}})) return 1;                 // leading, doubled and trailing blank lines
    if (!good("4\r\n5\r\n\r\n8\r\n", {{4, 5}, {8}})) return 1;                      // CR LF
    if (!good("  4 \n\t5\t\n \t \n8", {{4, 5}, {8}})) return 1;
    if (!good("0010\n11\n", {{10, 11}})) return 1;
    if (!good("1\n\n4294967294\n", {{1}, {4294967294u}})) return 1;
    {   // every block size around a seeded random file, written as -F writes it
        std::mt19937_64 rng(20263);
        for (int rep = 0; rep < 200; ++rep) {
            std::vector<std::vector<uint32_t>> want;
            std::string text;
            uint32_t g = (uint32_t)(rng() % 5);
            const size_t blocks = 1 + rng() % 9;
            for (size_t b = 0; b < blocks; ++b) {
                if (b) text += '\n';
                want.emplace_back();
                const size_t m = 1 + rng() % 70;
                for (size_t i = 0; i < m; ++i) { want.back().push_back(g); text += std::to_string(g) + "\n"; g += 1 + (uint32_t)(rng() % 3); }
                g += (uint32_t)(rng() % 40);
            }
            if (!good(text, want)) return 1;
        }
    }
    // ---- every refusal, with the line
    if (!bad("", "lists no genome ids")) return 1;
    if (!bad("\n\n \r\n", "lists no genome ids")) return 1;
    if (!bad("1\n2\nx\n", "line 3 ")) return 1;
    if (!bad("1\n2 3\n", "line 2 ")) return 1;
    if (!bad("-1\n", "line 1 ")) return 1;
    if (!bad("1\n\n+2\n", "line 3 ")) return 1;
    if (!bad("1\n0x10\n", "line 2 ")) return 1;
    if (!bad("1\n2.0\n", "line 2 ")) return 1;
    if (!bad("4294967295\n", "line 1 ")) return 1;                                  // (the left-out mark is no id)
    if (!bad("4294967296\n", "line 1 ")) return 1;
    if (!bad("99999999999\n", "line 1 ")) return 1;
    if (!bad("1\n99999999999999999999999999\n", "line 2 ")) return 1;
    if (!bad("5\n4\n", "line 2 ")) return 1;                                        // a decreasing id
    if (!bad("1\n2\n\n3\n2\n", "line 5 ")) return 1;
    if (!bad("1\n2\n\n0\n", "line 4 ")) return 1;                                   // ... across a blank line
    if (!bad("5\n5\n", "line 2 ")) return 1;                                        // an equal id
    if (!bad("1\r\n\r\n1\r\n", "line 3 ")) return 1;
    // ---- the writer
    std::mt19937_64 rng(20262);
    for (uint32_t n = 0; n <= 70; ++n)
        for (int rep = 0; rep < 20; ++rep) {
            std::vector<mk_clade_tally> t(n);
            std::vector<uint32_t> first(n), members(n);
            uint32_t g = 0;
            for (uint32_t c = 0; c < n; ++c) {
                mk_clade_tally &x = t[c];
                x.listed = rng() % 3 ? rng() % 1000 : 0;
                x.unique = x.listed ? rng() % (x.listed + 1) : 0;
                x.best = x.listed ? rng() % (x.listed + 1) : 0;
                x.best_matches = x.best * (rng() % 4096);
                x.hits = x.listed * (1 + rng() % 64);
                g += (uint32_t)(rng() % 5);
                first[c] = g;
                members[c] = 1 + (uint32_t)(rng() % 64);
                g += members[c];
            }
            if (!same(t, first, members, rng() % 100000)) return 1;
        }
    for (uint32_t n : {1u, 304u, 5000u}) {
        std::vector<mk_clade_tally> none(n, mk_clade_tally{0, 0, 0, 0, 0}), all(n, mk_clade_tally{3, 1, 2, 900, 7});
        std::vector<uint32_t> first(n), members(n, 2);
        for (uint32_t c = 0; c < n; ++c) first[c] = 2 * c;
        if (!same(none, first, members, 0) || !same(all, first, members, 3ull * n)) return 1;
    }
    {   // counters beyond 32 bits, and the largest there are
        std::vector<mk_clade_tally> t(3, mk_clade_tally{1ull << 40, 1ull << 33, 1ull << 39, 1ull << 52, 1ull << 46});
        t[1] = mk_clade_tally{UINT64_MAX, 0, UINT64_MAX, UINT64_MAX, UINT64_MAX};
        if (!same(t, {0, 4294967290u, 4294967293u}, {4294967290u, 3, 2}, 1ull << 41)) return 1;
    }
    printf("ok %u\n", cases);
    return 0;
}
