// The file of `miekki -G`: the greedy gather over the cover table of a read set (mk_cover_gather) -- the genome that explains
// most of what is still unexplained, its cells struck from the sample, and again, until no genome explains min_new cells.  One
// line per pick, IN PICK ORDER: <id> TAB <fresh> TAB <covered> TAB <sketch_size>, and with -D's table a fifth field TAB
// <depth_sum>.  fresh is what the genome explains that no pick before it did, covered its overlap with the whole sample;
// depth_sum / fresh is the mean depth of what the genome alone explains.  With 8-bit fingerprints an unrelated genome's fresh
// is about sketch_size * live cells / (P * 256): -g has to stand clear of it.  Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>

#include "miekki_hip.h"

namespace mkhost {

// picks[0 .. n) as mk_cover_gather returns them; `text` is appended to; returns the sum of fresh
inline uint64_t format_gather(const mk_pick *picks, uint64_t n, bool with_depth, std::string &text)
{
    uint64_t explained = 0;
    for (uint64_t i = 0; i < n; ++i) {
        text += std::to_string(picks[i].genome); text += '\t';
        text += std::to_string(picks[i].fresh); text += '\t';
        text += std::to_string(picks[i].covered); text += '\t';
        text += std::to_string(picks[i].sketch_size);
        if (with_depth) { text += '\t'; text += std::to_string(picks[i].depth_sum); }
        text += '\n';
        explained += picks[i].fresh;
    }
    return explained;
}

inline std::string gather_summary(uint64_t queries, uint64_t explained, uint64_t cells, uint64_t genomes, uint32_t min_new)
{
    return "gather: " + std::to_string(queries) + " queries, " + std::to_string(explained) + " of " + std::to_string(cells) +
           " seen cells explained by " + std::to_string(genomes) + " genomes, each at least " + std::to_string(min_new) + " new";
}

}  // namespace mkhost
