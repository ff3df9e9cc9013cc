// host/families.hpp against a restatement that shares nothing with it (a map of sorted sets), on seeded random partitions of
// every small size, on the shapes a collection has (one family, all singletons, a 300-clique among others) and on labels
// that are none -- built under AddressSanitizer + UBSan by tests/test_families_abi.py.  Prints "ok <cases>".
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "families.hpp"

static std::string restated(const std::vector<uint32_t> &labels, mkhost::FamilyCounts &c)
{
    std::map<uint32_t, std::set<uint32_t>> fam;
    for (uint32_t j = 0; j < labels.size(); ++j) fam[labels[j]].insert(j);
    std::string out;
    c = mkhost::FamilyCounts();
    bool first = true;
    for (const auto &f : fam) {
        if (!first) out += "\n";
        first = false;
        for (uint32_t j : f.second) out += std::to_string(j) + "\n";
        ++c.families;
        if (f.second.size() == 1) ++c.singletons;
        if (f.second.size() > c.largest) c.largest = f.second.size();
    }
    return out;
}

static bool same(const std::vector<uint32_t> &labels)
{
    mkhost::FamilyCounts a, b;
    std::string text = "kept", why;
    if (!mkhost::format_families(labels.data(), labels.size(), text, a, why)) { printf("refused: %s\n", why.c_str()); return false; }
    const std::string want = "kept" + restated(labels, b);
    if (text != want || a.families != b.families || a.largest != b.largest || a.singletons != b.singletons) { printf("differs at n = %zu\n", labels.size()); return false; }
    const std::string line = mkhost::family_summary(a);
    return line == "families: " + std::to_string(b.families) + ", largest " + std::to_string(b.largest) + ", singletons " + std::to_string(b.singletons);
}

int main()
{
    std::mt19937_64 rng(20260);
    unsigned cases = 0;
    for (uint32_t n = 0; n <= 70; ++n)
        for (int rep = 0; rep < 20; ++rep, ++cases) {
            // a random partition: every genome joins an earlier genome's family or starts one
            std::vector<uint32_t> labels(n);
            for (uint32_t j = 0; j < n; ++j) labels[j] = (j && rng() % 3) ? labels[rng() % j] : j;
            if (!same(labels)) return 1;
        }
    for (uint32_t n : {1u, 304u, 5000u}) {
        std::vector<uint32_t> one(n, 0), all(n);
        for (uint32_t j = 0; j < n; ++j) all[j] = j;
        if (!same(one) || !same(all)) return 1;
        cases += 2;
    }
    {   // dups' shape: genome 0 alone, a 300-clique labelled 1 with three strangers in between
        std::vector<uint32_t> labels(304, 1);
        for (uint32_t j : {0u, 52u, 150u, 248u}) labels[j] = j;
        if (!same(labels)) return 1;
        ++cases;
    }
    // labels that are none: beyond the ids, above their genome, not a root
    for (const std::vector<uint32_t> &bad : {std::vector<uint32_t>{0, 5}, std::vector<uint32_t>{1, 1}, std::vector<uint32_t>{0, 0, 1}, std::vector<uint32_t>{0xffffffffu}}) {
        mkhost::FamilyCounts c;
        std::string text, why;
        if (mkhost::format_families(bad.data(), bad.size(), text, c, why) || why.empty() || !text.empty()) { printf("accepted labels that are none\n"); return 1; }
        ++cases;
    }
    printf("ok %u\n", cases);
    return 0;
}
