// The files of `miekki -S <list> -c <file>`: the cover of a cohort -- the read files the list names, one sample each, eight
// samples per table and pass over the matrix (mk_qset_run_panel, mk_panel_count).  The -c file has one line per (sample,
// genome) with at least one covered fingerprint, samples ascending and ids ascending within a sample:
// <sample> TAB <id> TAB <covered> TAB <sketch_size> -- sample s's lines without their first field are the -C file of a run
// with -a on that sample's file.  Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace mkhost {

// the list's lines of more than 3 characters, as -A's list is read (a trailing carriage return is not part of a name)
inline void panel_list_files(const std::string &text, std::vector<std::string> &files)
{
    size_t at = 0;
    while (at < text.size()) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        std::string line = text.substr(at, end - at);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.size() > 3) files.push_back(line);
        at = end + 1;
    }
}

// covered[j], sketch_size[j] = those of genome j for this sample, ids starting at 0; `text` is appended to; returns the lines written
inline uint64_t format_panel(uint64_t sample, const uint32_t *covered, const uint32_t *sketch_size, uint64_t n, std::string &text)
{
    const std::string first = std::to_string(sample) + '\t';
    uint64_t genomes = 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (!covered[j]) continue;
        text += first;
        text += std::to_string(j); text += '\t';
        text += std::to_string(covered[j]); text += '\t';
        text += std::to_string(sketch_size[j]); text += '\n';
        ++genomes;
    }
    return genomes;
}

// h, fp_bits: the index's; P * 2^fp_bits cells in all
inline std::string panel_sample_summary(uint64_t sample, uint64_t queries, uint64_t cells, uint32_t h, uint32_t fp_bits, uint64_t genomes)
{
    return "panel[" + std::to_string(sample) + "]: " + std::to_string(queries) + " queries, " + std::to_string(cells) + " of " +
           std::to_string(1ull << (h + fp_bits)) + " cells seen, " + std::to_string(genomes) + " genomes covered";
}

inline std::string panel_summary(uint64_t samples, uint64_t slots)
{
    return "panel: " + std::to_string(samples) + " samples, " + std::to_string((samples + slots - 1) / slots) + " passes over the matrix";
}

}  // namespace mkhost
