// The files of `miekki -J <levels> -H <taxonomy> -O <order>`: the nested families of the indexed genomes at several thresholds
// (mk_index_hierarchy) laid out as what the read-placing flags take -- an order in which every family of every level is a run
// of ids (-O: a list for -K) and the taxonomy over the NEW ids, the places in that order (-H: a file for -T).
//   * the order: the genomes sorted by the key (label at level 0, ..., label at level L-1, old id); levels nest, so the
//     family of a genome at level l is the run of places that share its labels 0 .. l;
//   * the nodes, in the preorder parse_taxonomy (taxonomy.hpp) demands -- ascending first id, among equal first ids the larger
//     last id first: a family of level l gets a node when it has at least two members and (l == 0 or) its run differs from
//     the run of the level l-1 family around it -- a family that stays the same through several levels is ONE node, named
//     for the loosest of them -- and every genome gets a leaf <p> <p>;
//   * the names: L<l>.<label> for a family, <label> its smallest old id; g<old id> for a leaf.
// -O has one decimal old id per line, -H one `<first> <last> <name>` per line.  Plain C++, no GPU in it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "miekki_hip.h"                         // mk_level, MK_MAX_LEVELS: the header alone

namespace mkhost {

// The argument of -J: a comma-separated list of 1 .. MK_MAX_LEVELS levels, the loosest first, each <min_score> or
// <min_score>:<min_intersection> -- plain decimals, the score a whole number, the intersection with or without a fraction; a
// level without an intersection takes `default_inter` (-F's, 0.5 * -s).  False (and why, the level named) for anything else
// and for a score or an intersection below the level's before it.
inline bool parse_levels(const std::string &arg, double default_inter, std::vector<mk_level> &levels, std::string &why)
{
    levels.clear();
    auto digits = [](const std::string &s) { return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos; };
    for (size_t at = 0; at <= arg.size();) {
        size_t end = arg.find(',', at);
        if (end == std::string::npos) end = arg.size();
        const std::string item = arg.substr(at, end - at), here = "-J: level " + std::to_string(levels.size());
        at = end + 1;
        if (levels.size() == MK_MAX_LEVELS) { why = "-J takes at most " + std::to_string(MK_MAX_LEVELS) + " levels"; return false; }
        const size_t colon = item.find(':');
        const std::string score = item.substr(0, colon), inter = colon == std::string::npos ? std::string() : item.substr(colon + 1);
        const size_t dot = inter.find('.');
        const bool inter_ok = colon == std::string::npos || (inter.size() <= 300 && digits(inter.substr(0, dot)) && (dot == std::string::npos || digits(inter.substr(dot + 1))));
        if (!digits(score) || score.size() > 10 || strtoull(score.c_str(), nullptr, 10) > 0xffffffffull || !inter_ok) {
            why = here + " is not <min_score> or <min_score>:<min_intersection>: '" + item + "'";
            return false;
        }
        mk_level lv{(uint32_t)strtoull(score.c_str(), nullptr, 10), 0, colon == std::string::npos ? default_inter : strtod(inter.c_str(), nullptr)};
        if (!levels.empty() && lv.min_score < levels.back().min_score) {
            why = here + ": min_score " + score + " is below the level's before it: the levels go from the loosest to the strictest";
            return false;
        }
        if (!levels.empty() && lv.min_intersection < levels.back().min_intersection) {
            why = here + ": min_intersection " + (colon == std::string::npos ? std::to_string(default_inter) : inter) + " is below the level's before it: the levels go from the loosest to the strictest";
            return false;
        }
        levels.push_back(lv);
    }
    return true;
}

struct HierarchyNode {
    uint32_t first = 0, last = 0;      // places, both inclusive
    uint32_t depth = 0;                // the number of nodes around it
    std::string name;
};

// labels[l * G + j] = the label of genome j at level l (ids starting at 0), level 0 the loosest.  False (and why) for labels
// that are no family labels at some level (format_families' test: a label is the smallest id of its family) and for levels
// that do not nest: two genomes that share a label at level l but not at level l - 1.  order[p] = the old id that goes to
// place p.
inline bool layout_hierarchy(const uint32_t *labels, uint32_t L, uint64_t G, std::vector<uint32_t> &order, std::vector<HierarchyNode> &nodes, std::string &why)
{
    order.clear();
    nodes.clear();
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t *lab = labels + (uint64_t)l * G;
        for (uint64_t j = 0; j < G; ++j) {
            const uint64_t r = lab[j];
            if (r > j || lab[r] != r) {
                why = "level " + std::to_string(l) + ": genome " + std::to_string(j) + " carries label " + std::to_string(r) + ", which is not the smallest id of a family";
                return false;
            }
            // (j and its family's smallest id r under one label of the level above: so are all of the family)
            if (l && (lab - G)[j] != (lab - G)[r]) {
                why = "level " + std::to_string(l) + ": genomes " + std::to_string(r) + " and " + std::to_string(j) + " share label " + std::to_string(r) +
                      " but not a label at level " + std::to_string(l - 1) + ": the levels do not nest";
                return false;
            }
        }
    }
    order.resize(G);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        for (uint32_t l = 0; l < L; ++l) {
            const uint32_t lx = labels[(uint64_t)l * G + x], ly = labels[(uint64_t)l * G + y];
            if (lx != ly) return lx < ly;
        }
        return x < y;
    });
    // per level and place: where the run of the place's family starts and ends (nested levels: a run of one label)
    std::vector<uint32_t> first((uint64_t)L * G), last((uint64_t)L * G);
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t *lab = labels + (uint64_t)l * G;
        uint32_t *f = first.data() + (uint64_t)l * G, *e = last.data() + (uint64_t)l * G;
        for (uint64_t p = 0; p < G; ++p) f[p] = p && lab[order[p]] == lab[order[p - 1]] ? f[p - 1] : (uint32_t)p;
        for (uint64_t p = G; p-- > 0;) e[p] = p + 1 < G && lab[order[p]] == lab[order[p + 1]] ? e[p + 1] : (uint32_t)p;
    }
    std::vector<uint32_t> open;                                  // the last places of the nodes around the current place
    for (uint64_t p = 0; p < G; ++p) {
        while (!open.empty() && open.back() < p) open.pop_back();
        for (uint32_t l = 0; l < L; ++l) {
            const uint64_t at = (uint64_t)l * G + p;
            if (first[at] != p || last[at] == p) continue;                                       // not a family's first place; a family of one
            if (l && first[at - G] == first[at] && last[at - G] == last[at]) continue;           // the family of the level above, unchanged
            nodes.push_back({(uint32_t)p, last[at], (uint32_t)open.size(), "L" + std::to_string(l) + "." + std::to_string(labels[(uint64_t)l * G + order[p]])});
            open.push_back(last[at]);
        }
        nodes.push_back({(uint32_t)p, (uint32_t)p, (uint32_t)open.size(), "g" + std::to_string(order[p])});
    }
    return true;
}

// -O: `text` is appended to
inline void format_hierarchy_order(const std::vector<uint32_t> &order, std::string &text)
{
    for (uint32_t id : order) { text += std::to_string(id); text += '\n'; }
}

// -H: `text` is appended to
inline void format_hierarchy_taxonomy(const std::vector<HierarchyNode> &nodes, std::string &text)
{
    for (const HierarchyNode &v : nodes) {
        text += std::to_string(v.first); text += ' ';
        text += std::to_string(v.last); text += ' ';
        text += v.name; text += '\n';
    }
}

// hierarchy: <L> levels, <n0>/<n1>/.../<nL-1> families, <nodes> nodes, depth <max depth + 1>
inline std::string hierarchy_summary(const uint32_t *labels, uint32_t L, uint64_t G, const std::vector<HierarchyNode> &nodes)
{
    std::string s = "hierarchy: " + std::to_string(L) + " levels, ";
    for (uint32_t l = 0; l < L; ++l) {
        uint64_t n = 0;
        for (uint64_t j = 0; j < G; ++j) n += labels[(uint64_t)l * G + j] == j;
        if (l) s += '/';
        s += std::to_string(n);
    }
    uint32_t deepest = 0;
    for (const HierarchyNode &v : nodes) deepest = std::max(deepest, v.depth + 1);
    return s + " families, " + std::to_string(nodes.size()) + " nodes, depth " + std::to_string(deepest);
}

}  // namespace mkhost
