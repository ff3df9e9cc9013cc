// The file of `miekki -E`: abundance by expectation-maximisation over the reads that several genomes share (mk_qset_run_share,
// mk_share_rounds) -- a read whose genomes within -w percent of its best one are several is split among them in proportion to
// what the other reads say about them, -I times.  One line per genome that a read is settled on or shared by, ascending id:
// <id> TAB <reads> TAB <unique> TAB <shared>.  reads is the genome's abundance, counted in reads with 32 fractional bits, printed
// as <whole>.<three digits>, the digits cut, not rounded: integers only, so the bytes follow from the counters.  unique are the
// reads settled on the genome, shared those it shares with others.  Genome length plays no part.  Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "miekki_hip.h"

namespace mkhost {

// a count of reads with 32 fractional bits as <whole>.<three digits>
inline std::string reads_text(uint64_t a)
{
    char buf[40];
    snprintf(buf, sizeof buf, "%llu.%03u", (unsigned long long)(a >> 32), (unsigned)(((a & 0xffffffffull) * 1000) >> 32));
    return buf;
}

// abundance, unique, shared [n] as mk_share_rounds and mk_share_export return them; `text` is appended to; returns the lines
inline uint64_t format_abundance(const uint64_t *abundance, const uint64_t *unique, const uint64_t *shared, uint64_t n, uint32_t id_base, std::string &text)
{
    uint64_t genomes = 0;
    for (uint64_t g = 0; g < n; ++g) {
        if (!unique[g] && !shared[g]) continue;
        text += std::to_string(g + id_base); text += '\t';
        text += reads_text(abundance[g]); text += '\t';
        text += std::to_string(unique[g]); text += '\t';
        text += std::to_string(shared[g]); text += '\n';
        ++genomes;
    }
    return genomes;
}

inline std::string abundance_summary(const mk_share_info &info, uint64_t genomes, const mk_share_result &res, uint32_t margin)
{
    return "abundance: " + std::to_string(info.queries) + " queries, " + std::to_string(info.assigned) + " assigned, " +
           std::to_string(info.shared_reads) + " shared by several genomes, " + std::to_string(info.entries) + " ids stored, " +
           std::to_string(genomes) + " genomes listed, " + std::to_string(res.rounds) + " rounds, margin " + std::to_string(margin) +
           ", last change " + reads_text(res.delta);
}

}  // namespace mkhost
