// The file of `miekki -C`: breadth of coverage of the indexed genomes by a read set (mk_qset_run_cover, mk_cover_count), one line
// per genome with at least one covered fingerprint, in ascending id: <id> TAB <covered> TAB <sketch_size>.  With 8-bit
// fingerprints an unrelated genome is covered at about cells / (P * 256) of its sketch by chance: the summary line gives the
// cells for that reason.  Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>

namespace mkhost {

// covered[j], sketch_size[j] = those of genome j, ids starting at 0; `text` is appended to; returns the lines written
inline uint64_t format_cover(const uint32_t *covered, const uint32_t *sketch_size, uint64_t n, std::string &text)
{
    uint64_t genomes = 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (!covered[j]) continue;
        text += std::to_string(j); text += '\t';
        text += std::to_string(covered[j]); text += '\t';
        text += std::to_string(sketch_size[j]); text += '\n';
        ++genomes;
    }
    return genomes;
}

// h, fp_bits: the index's; P * 2^fp_bits cells in all
inline std::string cover_summary(uint64_t queries, uint64_t cells, uint32_t h, uint32_t fp_bits, uint64_t genomes)
{
    return "cover: " + std::to_string(queries) + " queries, " + std::to_string(cells) + " of " + std::to_string(1ull << (h + fp_bits)) +
           " cells seen, " + std::to_string(genomes) + " genomes covered";
}

}  // namespace mkhost
