// Stand-alone driver of host/taxonomy.hpp's -V writer for tests/test_markers_abi.py (built there with AddressSanitizer and
// UBSan; no GPU):
//   markers_check <taxonomy file> <counts>   the -V bytes and the summary line (99 queries) for counters given as text, specific
//                                            and covered per node and then of the slot above every node; "refused: <why>" for a
//                                            file that is no taxonomy
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
    std::vector<mk_node_markers> nm(t.lo.size() + 1);
    std::istringstream in(slurp(argv[2]));
    for (auto &r : nm) in >> r.specific >> r.covered;
    std::string text;
    const mkhost::MarkerCounts counts = mkhost::format_markers(nm.data(), t, text);
    std::cout << text << mkhost::markers_summary(99, counts) << "\n";
    return 0;
}
