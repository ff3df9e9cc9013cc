// Stand-alone driver of host/taxonomy.hpp's -U writer for tests/test_taxon_cover_abi.py (built there with AddressSanitizer and
// UBSan; no GPU):
//   taxon_cover_check <taxonomy file> <counts>   the -U bytes and the summary line (99 queries, 1234 cells, -h 9, 8 bits) for
//                                                counters given as text, held and covered per node; "refused: <why>" for a
//                                                file that is no taxonomy
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
    mkhost::Taxonomy t;
    std::string why;
    if (!mkhost::parse_taxonomy(slurp(argv[1]), argv[1], t, why)) { std::cout << "refused: " << why << "\n"; return 0; }
    std::vector<mk_node_cover> nc(t.lo.size());
    std::istringstream in(slurp(argv[2]));
    for (auto &r : nc) in >> r.held >> r.covered;
    std::string text;
    const uint64_t nodes = mkhost::format_taxon_cover(nc.data(), t, text);
    std::cout << text << mkhost::taxon_cover_summary(99, 1234, 9, 8, nodes, nc.size()) << "\n";
    return 0;
}
