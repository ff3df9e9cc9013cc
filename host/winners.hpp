// The file of `miekki -W`: the winner-takes-all screen of the indexed genomes by a read set (mk_cover_winners) -- every seen
// cell credited to the best-contained genome that holds it -- one line per genome that wins at least one cell, in ascending id:
// <id> TAB <won> TAB <covered> TAB <sketch_size>.  Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>

namespace mkhost {

// won[j], covered[j], sketch_size[j] = those of genome j, ids starting at 0; `text` is appended to; returns the lines written
inline uint64_t format_winners(const uint32_t *won, const uint32_t *covered, const uint32_t *sketch_size, uint64_t n, std::string &text)
{
    uint64_t genomes = 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (!won[j]) continue;
        text += std::to_string(j); text += '\t';
        text += std::to_string(won[j]); text += '\t';
        text += std::to_string(covered[j]); text += '\t';
        text += std::to_string(sketch_size[j]); text += '\n';
        ++genomes;
    }
    return genomes;
}

inline std::string winners_summary(uint64_t queries, uint64_t claimed, uint64_t cells, uint64_t genomes)
{
    return "winners: " + std::to_string(queries) + " queries, " + std::to_string(claimed) + " of " + std::to_string(cells) +
           " seen cells held, " + std::to_string(genomes) + " genomes win cells";
}

}  // namespace mkhost
