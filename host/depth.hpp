// The file of `miekki -D`: depth of coverage of the indexed genomes by a read set (mk_qset_run_depth, mk_depth_profile), one
// line per genome with at least one covered fingerprint, in ascending id: <id> TAB <median> TAB <sum> TAB <covered> TAB
// <sketch_size>.  median is the lower median, over the covered fingerprints, of the number of reads that hold each (capped at
// 255: a median of 255 means "255 or more", and the summary line gives the cells at the cap for that reason); the mean depth is
// sum / covered.  With 8-bit fingerprints read a median only where covered / sketch_size stands clear of cells / (P * 256).
// Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>

#include "miekki_hip.h"

namespace mkhost {

// depth[j], sketch_size[j] = those of genome j, ids starting at 0; `text` is appended to; returns the lines written
inline uint64_t format_depth(const mk_depth *depth, const uint32_t *sketch_size, uint64_t n, std::string &text)
{
    uint64_t genomes = 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (!depth[j].covered) continue;
        text += std::to_string(j); text += '\t';
        text += std::to_string(depth[j].median); text += '\t';
        text += std::to_string(depth[j].sum); text += '\t';
        text += std::to_string(depth[j].covered); text += '\t';
        text += std::to_string(sketch_size[j]); text += '\n';
        ++genomes;
    }
    return genomes;
}

// h, fp_bits: the index's; P * 2^fp_bits cells in all
inline std::string depth_summary(uint64_t queries, uint64_t cells, uint64_t saturated, uint32_t h, uint32_t fp_bits, uint64_t genomes)
{
    return "depth: " + std::to_string(queries) + " queries, " + std::to_string(cells) + " of " + std::to_string(1ull << (h + fp_bits)) +
           " cells seen, " + std::to_string(saturated) + " at 255, " + std::to_string(genomes) + " genomes covered";
}

}  // namespace mkhost
