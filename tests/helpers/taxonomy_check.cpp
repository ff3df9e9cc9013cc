// Stand-alone driver of host/taxonomy.hpp for tests/test_lca_abi.py (built there with AddressSanitizer and UBSan; no GPU):
//   taxonomy_check parse <file>             "ok <n>" and a line per node, lo hi parent depth line |name|, or "refused: <why>"
//   taxonomy_check fits <file> <n_genomes>  "ok" or "refused: <why>"
//   taxonomy_check report <file> <counts>   the -y bytes and the summary line for counters given as text, three per slot
//   taxonomy_check reads <nodes...>         the -Y bytes for the nodes given (numbers, * or -), ordinals from 7
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "taxonomy.hpp"

static std::string slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    if (mode == "reads") {
        std::vector<uint32_t> nodes;
        for (int i = 2; i < argc; ++i) nodes.push_back(!strcmp(argv[i], "*") ? MK_LCA_ABOVE : !strcmp(argv[i], "-") ? MK_NO_NODE : (uint32_t)strtoul(argv[i], nullptr, 10));
        std::string text;
        mkhost::format_lca_reads(nodes.data(), nodes.size(), 7, text);
        std::cout << text;
        return 0;
    }
    mkhost::Taxonomy t;
    std::string why;
    if (!mkhost::parse_taxonomy(slurp(argv[2]), argv[2], t, why)) { std::cout << "refused: " << why << "\n"; return 0; }
    if (mode == "parse") {
        std::cout << "ok " << t.lo.size() << "\n";
        for (size_t v = 0; v < t.lo.size(); ++v)
            std::cout << t.lo[v] << " " << t.hi[v] << " " << (t.parent[v] == MK_NO_NODE ? -1 : (long)t.parent[v]) << " " << t.depth[v] << " " << t.line[v] << " |" << t.name[v] << "|\n";
    } else if (mode == "fits" && argc > 3) {
        if (mkhost::taxonomy_fits(t, argv[2], strtoull(argv[3], nullptr, 10), why)) std::cout << "ok\n";
        else std::cout << "refused: " << why << "\n";
    } else if (mode == "report" && argc > 3) {
        std::vector<mk_lca_tally> lt(t.lo.size() + 1);
        std::istringstream in(slurp(argv[3]));
        for (auto &r : lt) in >> r.reads >> r.best_matches >> r.hits;
        std::string text;
        mkhost::LcaCounts counts;
        mkhost::format_lca_report(lt.data(), t, text, counts);
        std::cout << text << mkhost::lca_summary(99, counts, 10) << "\n";
    } else {
        return 2;
    }
    return 0;
}
