// The file of `miekki -P`: the profile of a read set over the indexed genomes (mk_qset_run_tally), one line per genome that at
// least one query lists, in ascending id: <id> TAB <best> TAB <unique> TAB <listed> TAB <best_matches>.  Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>

#include "miekki_hip.h"

namespace mkhost {

struct ProfileCounts {
    uint64_t assigned = 0, unique = 0, genomes = 0;   // sum of best, sum of unique, lines written
};

// tally[j] = the counters of genome j, ids starting at 0; `text` is appended to
inline void format_profile(const mk_tally *tally, uint64_t n, std::string &text, ProfileCounts &counts)
{
    counts = ProfileCounts();
    for (uint64_t j = 0; j < n; ++j) {
        const mk_tally &t = tally[j];
        if (!t.listed) continue;
        text += std::to_string(j); text += '\t';
        text += std::to_string(t.best); text += '\t';
        text += std::to_string(t.unique); text += '\t';
        text += std::to_string(t.listed); text += '\t';
        text += std::to_string(t.best_matches); text += '\n';
        counts.assigned += t.best;
        counts.unique += t.unique;
        ++counts.genomes;
    }
}

inline std::string profile_summary(uint64_t queries, const ProfileCounts &c)
{
    return "profile: " + std::to_string(queries) + " queries, " + std::to_string(c.assigned) + " assigned, " + std::to_string(c.unique) +
           " listing one genome only, " + std::to_string(c.genomes) + " genomes listed";
}

}  // namespace mkhost
