// The writer of `miekki -E`'s file and line (host/abundance.hpp) as a stand-alone program, for tests/test_share_abi.py (built
// with -fsanitize=address,undefined):
//   abundance_check <counts file> <queries> <assigned> <shared_reads> <entries> <rounds> <margin> <delta>
// The counts file holds a line per genome: <abundance> <unique> <shared>, decimal 64-bit integers.  Prints the file's bytes,
// then the summary line.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "abundance.hpp"

int main(int argc, char **argv)
{
    if (argc != 9) { fprintf(stderr, "usage: see the head of abundance_check.cpp\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<uint64_t> abundance, unique, shared;
    uint64_t a, u, s;
    while (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &u, &s) == 3) { abundance.push_back(a); unique.push_back(u); shared.push_back(s); }
    fclose(f);
    auto num = [&](int i) { return (uint64_t)strtoull(argv[i], nullptr, 10); };
    const mk_share_info info{num(2), num(3), num(4), num(5)};
    const mk_share_result res{num(8), 0, (uint32_t)num(6), 0};
    std::string text;
    const uint64_t genomes = mkhost::format_abundance(abundance.data(), unique.data(), shared.data(), abundance.size(), 0, text);
    fwrite(text.data(), 1, text.size(), stdout);
    puts(mkhost::abundance_summary(info, genomes, res, (uint32_t)num(7)).c_str());
    return 0;
}
