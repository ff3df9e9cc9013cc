// host/hierarchy.hpp and the -J -H -O rules of host/options.hpp alone, without the library.
//     hierarchy_check layout <L> <G> <labels file> <order file> <taxonomy file>
// reads L * G labels (u32, level-major), lays them out and writes the two files; prints the summary line, then what
// parse_taxonomy makes of the taxonomy's text: `parsed <nodes>` and one line of the nodes' depths.  A refused layout or a
// taxonomy parse_taxonomy does not take: one line, `refused: <why>`, status 1.
//     hierarchy_check levels <argument> <default intersection>
// prints the levels of a -J argument, `<min_score> <min_intersection>` per line, or `refused: <why>` with status 1.
//     hierarchy_check refusal <devices> <rank_mode 0|1> <rank_id> <rank_world> miekki [miekki's arguments]
// prints the first refusal of the command line (nothing for an accepted one); status 1 for a refusal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>

#include "options.hpp"

static int refused(const std::string &why)
{
    std::cout << "refused: " << why << std::endl;
    return 1;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "layout" && argc == 7) {
        const uint32_t L = (uint32_t)atol(argv[2]);
        const uint64_t G = (uint64_t)atoll(argv[3]);
        std::ifstream in(argv[4], std::ios::binary);
        const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (raw.size() != (size_t)L * G * 4) { std::cerr << "labels file: " << raw.size() << " bytes" << std::endl; return 2; }
        std::vector<uint32_t> labels((size_t)L * G);
        if (!raw.empty()) memcpy(labels.data(), raw.data(), raw.size());
        std::vector<uint32_t> order;
        std::vector<mkhost::HierarchyNode> nodes;
        std::string why, text;
        if (!mkhost::layout_hierarchy(labels.data(), L, G, order, nodes, why)) return refused(why);
        mkhost::format_hierarchy_order(order, text);
        std::ofstream(argv[5], std::ios::binary) << text;
        text.clear();
        mkhost::format_hierarchy_taxonomy(nodes, text);
        std::ofstream(argv[6], std::ios::binary) << text;
        std::cout << mkhost::hierarchy_summary(labels.data(), L, G, nodes) << std::endl;
        mkhost::Taxonomy tax;
        if (!mkhost::parse_taxonomy(text, "tax", tax, why)) return refused(why);
        if (!mkhost::taxonomy_fits(tax, "tax", G, why)) return refused(why);
        std::cout << "parsed " << tax.lo.size() << std::endl;
        for (size_t v = 0; v < tax.depth.size(); ++v) std::cout << (v ? " " : "") << tax.depth[v];
        std::cout << std::endl;
        return 0;
    }
    if (mode == "levels" && argc == 4) {
        std::vector<mk_level> levels;
        std::string why;
        if (!mkhost::parse_levels(argv[2], atof(argv[3]), levels, why)) return refused(why);
        for (const mk_level &lv : levels) printf("%u %.17g\n", lv.min_score, lv.min_intersection);
        return 0;
    }
    if (mode == "refusal" && argc >= 7) {
        mkhost::Where where;
        where.devices = (size_t)atol(argv[2]);
        where.rank_mode = atoi(argv[3]) != 0;
        where.rank_id = atoi(argv[4]);
        where.rank_world = atoi(argv[5]);
        mkhost::Options opt;
        mkhost::parse_options(argc - 6, argv + 6, opt);
        mkhost::Checked got;
        const std::string no = mkhost::refusal(opt, where, got);
        std::cout << no << std::endl;
        for (const mk_level &lv : got.levels) printf("%u %.17g\n", lv.min_score, lv.min_intersection);
        return no.empty() ? 0 : 1;
    }
    std::cerr << "usage: hierarchy_check layout|levels|refusal ..." << std::endl;
    return 2;
}
