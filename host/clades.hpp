// The files of `miekki -L <clades> -p <file>`: the profile of a read set by clade (mk_qset_run_clade_tally).
// -L is read in -F's layout: one decimal genome id per line, blank lines between clades, the clade number = the block's index
// from 0; ids strictly increasing through the whole file (so clade numbers never decrease along the ids: the one restriction
// of a clade map); genomes the file does not name are left out.  -p gets one line per clade that some read lists, ascending:
// <clade> TAB <first_id> TAB <members> TAB <best> TAB <unique> TAB <listed> TAB <best_matches> TAB <hits>.
// Plain C++, no GPU in it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "miekki_hip.h"

namespace mkhost {

struct CladeList {
    std::vector<uint32_t> ids;       // the genomes named, strictly increasing
    std::vector<uint32_t> clade;     // clade[i] = the clade of ids[i], non-decreasing, from 0 without gaps
    std::vector<uint32_t> first_id;  // per clade: its smallest id
    std::vector<uint32_t> members;   // per clade: how many genomes it names
};

// `text` = the file's bytes, `name` = what the messages call it.  Lines may end in CR LF and carry blanks around the id; any
// number of blank lines is one separator, blank lines before the first id and after the last are ignored.  False (and why,
// with the line) for anything that is not an id, an id that does not exceed the one before, or a file without ids.
inline bool parse_clades(const std::string &text, const std::string &name, CladeList &out, std::string &why)
{
    out = CladeList();
    bool gap = false;                                            // a blank line since the last id
    uint64_t line_no = 0;
    for (size_t at = 0; at < text.size();) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        ++line_no;
        size_t b = at, e = end;
        auto blank = [](char ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f'; };
        while (b < e && blank(text[b])) ++b;
        while (e > b && blank(text[e - 1])) --e;
        at = end + 1;
        if (b == e) { gap = true; continue; }
        uint64_t v = 0;
        bool digits = e - b <= 10;
        for (size_t i = b; i < e && digits; ++i) {
            if (text[i] < '0' || text[i] > '9') digits = false;
            else v = v * 10 + (uint64_t)(text[i] - '0');
        }
        if (!digits || v >= 0xffffffffull) { why = "-L: line " + std::to_string(line_no) + " of " + name + " is not a genome id: " + text.substr(b, e - b); return false; }
        if (!out.ids.empty() && v <= out.ids.back()) {
            why = "-L: line " + std::to_string(line_no) + " of " + name + ": genome id " + std::to_string(v) + " does not exceed the one before, " +
                  std::to_string(out.ids.back()) + " (ids are strictly increasing: group the index with -K first)";
            return false;
        }
        if (out.ids.empty() || gap) { out.first_id.push_back((uint32_t)v); out.members.push_back(0); }
        gap = false;
        out.ids.push_back((uint32_t)v);
        out.clade.push_back((uint32_t)out.first_id.size() - 1);
        ++out.members.back();
    }
    if (out.ids.empty()) { why = "-L: " + name + " lists no genome ids"; return false; }
    return true;
}

// map[j] = the clade of genome j < n_genomes, MK_NO_CLADE where the list does not name it.  False (and why) for an id the
// index does not hold.
inline bool clade_map_of(const CladeList &list, uint64_t n_genomes, std::vector<uint32_t> &map, std::string &why)
{
    map.assign(n_genomes, MK_NO_CLADE);
    for (size_t i = 0; i < list.ids.size(); ++i) {
        if (list.ids[i] >= n_genomes) { why = "-L: genome id " + std::to_string(list.ids[i]) + " is beyond the index's " + std::to_string(n_genomes) + " genomes"; return false; }
        map[list.ids[i]] = list.clade[i];
    }
    return true;
}

struct CladeCounts {
    uint64_t assigned = 0, unique = 0, clades = 0;   // sum of best, sum of unique, lines written
};

// ct[c] = the counters of clade c, first_id[c] and members[c] as parse_clades left them; `text` is appended to
inline void format_clade_profile(const mk_clade_tally *ct, const uint32_t *first_id, const uint32_t *members, uint64_t n, std::string &text, CladeCounts &counts)
{
    counts = CladeCounts();
    for (uint64_t c = 0; c < n; ++c) {
        const mk_clade_tally &t = ct[c];
        if (!t.listed) continue;
        text += std::to_string(c); text += '\t';
        text += std::to_string(first_id[c]); text += '\t';
        text += std::to_string(members[c]); text += '\t';
        text += std::to_string(t.best); text += '\t';
        text += std::to_string(t.unique); text += '\t';
        text += std::to_string(t.listed); text += '\t';
        text += std::to_string(t.best_matches); text += '\t';
        text += std::to_string(t.hits); text += '\n';
        counts.assigned += t.best;
        counts.unique += t.unique;
        ++counts.clades;
    }
}

inline std::string clade_summary(uint64_t queries, const CladeCounts &c)
{
    return "clades: " + std::to_string(queries) + " queries, " + std::to_string(c.assigned) + " assigned, " + std::to_string(c.unique) +
           " listing one clade only, " + std::to_string(c.clades) + " clades listed";
}

}  // namespace mkhost
