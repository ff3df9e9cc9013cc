// The file of `miekki -F`: the families of the indexed genomes (mk_index_families), one decimal genome id per line, families in
// ascending order of their label (their smallest id), members ascending, one blank line between families -- a list -K takes
// as it is (it ignores blank lines) and that puts every family's genomes next to each other.  Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace mkhost {

struct FamilyCounts {
    uint64_t families = 0, largest = 0, singletons = 0;
};

// labels[j] = the label of genome j's family, ids starting at 0: a label is the family's smallest id, so labels[j] <= j and
// labels[labels[j]] == labels[j].  False (and why) for labels that are none; `text` is appended to.
inline bool format_families(const uint32_t *labels, uint64_t n, std::string &text, FamilyCounts &counts, std::string &why)
{
    counts = FamilyCounts();
    std::vector<uint64_t> at(n + 1, 0);                        // members per label, then where a label's members start
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t l = labels[j];
        if (l > j || labels[l] != l) { why = "genome " + std::to_string(j) + " carries label " + std::to_string(l) + ", which is not the smallest id of a family"; return false; }
        ++at[l + 1];
    }
    for (uint64_t l = 0; l < n; ++l) {
        const uint64_t m = at[l + 1];
        if (m) { ++counts.families; counts.singletons += m == 1; if (m > counts.largest) counts.largest = m; }
        at[l + 1] += at[l];
    }
    std::vector<uint32_t> member(n);
    std::vector<uint64_t> next(at.begin(), at.end() - 1);
    for (uint64_t j = 0; j < n; ++j) member[next[labels[j]]++] = (uint32_t)j;     // ascending j: members ascending
    bool first = true;
    for (uint64_t l = 0; l < n; ++l) {
        if (at[l] == at[l + 1]) continue;
        if (!first) text += '\n';
        first = false;
        for (uint64_t i = at[l]; i < at[l + 1]; ++i) { text += std::to_string(member[i]); text += '\n'; }
    }
    return true;
}

inline std::string family_summary(const FamilyCounts &c)
{
    return "families: " + std::to_string(c.families) + ", largest " + std::to_string(c.largest) + ", singletons " + std::to_string(c.singletons);
}

}  // namespace mkhost
