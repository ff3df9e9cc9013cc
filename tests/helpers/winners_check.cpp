// The order of the winner-takes-all screen (miekki_amd/csrc/cover_order.hpp) and the writer of `miekki -W` (host/winners.hpp) on
// crafted inputs, as a stand-alone program built under AddressSanitizer + UBSan by tests/test_winners_abi.py, which compares
// what is printed here with tests/winners_ref.py.  Per case: "case <name>", "cov ...", "ss ...", "order ...", "rank ...", the
// file's lines between "file" and "end", and the summary line.
#include <cinttypes>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "cover_order.hpp"
#include "winners.hpp"

static void row(const char *name, const std::vector<uint32_t> &v)
{
    printf("%s", name);
    for (uint32_t x : v) printf(" %" PRIu32, x);
    printf("\n");
}

static bool show(const char *name, const std::vector<uint32_t> &cov, const std::vector<uint32_t> &ss)
{
    const uint32_t n = (uint32_t)cov.size();
    std::vector<uint32_t> order(n), rank(n), again(n);
    mk::cover_order(cov.data(), ss.data(), n, order.data(), rank.data());
    mk::cover_order(cov.data(), ss.data(), n, again.data(), nullptr);          // (rank may be null)
    if (again != order) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (order[i] >= n || rank[order[i]] != i) return false;
    for (uint32_t i = 0; i + 1 < n; ++i)                                        // a strict order: neighbours one way only
        if (!mk::cover_before(cov[order[i]], ss[order[i]], order[i], cov[order[i + 1]], ss[order[i + 1]], order[i + 1]) ||
            mk::cover_before(cov[order[i + 1]], ss[order[i + 1]], order[i + 1], cov[order[i]], ss[order[i]], order[i]))
            return false;
    printf("case %s\n", name);
    row("cov", cov); row("ss", ss); row("order", order); row("rank", rank);
    // the writer, with won = the rank's parity times covered: some zero, some not
    std::vector<uint32_t> won(n);
    uint64_t claimed = 0;
    for (uint32_t g = 0; g < n; ++g) claimed += won[g] = rank[g] % 2 ? 0 : cov[g];
    row("won", won);
    std::string text;
    const uint64_t lines = mkhost::format_winners(won.data(), cov.data(), ss.data(), n, text);
    printf("file\n%send %" PRIu64 "\n%s\n", text.c_str(), lines, mkhost::winners_summary(3ull * n, claimed, claimed + 7, lines).c_str());
    return true;
}

int main()
{
    const uint32_t B = 1u << 28;
    bool ok = true;
    ok = ok && show("equal_shares_different_covered", {1, 2, 3, 50, 2, 0, 100}, {2, 4, 6, 100, 4, 9, 200});
    ok = ok && show("empty_sketches", {0, 5, 0, 0, 1, 0}, {0, 10, 7, 0, 1, 0});
    // products next to 2^56 that differ by one: beyond what a double tells apart
    ok = ok && show("products_near_2_56", {B - 2, B - 1, B - 1, B - 3, B, B - 2}, {B - 1, B, B - 1, B - 2, B, B - 1});
    ok = ok && show("products_near_2_64", {UINT32_MAX - 1, UINT32_MAX, UINT32_MAX - 2}, {UINT32_MAX, UINT32_MAX, UINT32_MAX - 1});
    ok = ok && show("all_equal", std::vector<uint32_t>(70, 33), std::vector<uint32_t>(70, 512));
    ok = ok && show("nothing_covered", std::vector<uint32_t>(9, 0), {5, 0, 3, 9, 1, 0, 7, 7, 2});
    ok = ok && show("no_genomes", {}, {});
    ok = ok && show("one_genome", {4}, {8});
    std::mt19937_64 rng(20263);
    for (int rep = 0; rep < 40 && ok; ++rep) {
        const uint32_t n = 1 + (uint32_t)(rng() % 300);
        std::vector<uint32_t> cov(n), ss(n);
        for (uint32_t j = 0; j < n; ++j) {
            ss[j] = rng() % 8 ? 1 + (uint32_t)(rng() % (rep % 2 ? 12 : 131072)) : 0;      // small sizes: many equal shares
            cov[j] = ss[j] ? (uint32_t)(rng() % (ss[j] + 1)) : 0;
        }
        ok = show(("random_" + std::to_string(rep)).c_str(), cov, ss);
    }
    if (!ok) { printf("FAILED\n"); return 1; }
    printf("ok\n");
    return 0;
}
