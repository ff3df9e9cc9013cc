// host/options.hpp alone, without the library: the first refusal of a command line as `miekki` would print it.
//     options_check <devices> <rank_mode 0|1> <rank_id> <rank_world> miekki [miekki's arguments]
// prints one line -- the refusal; nothing for an accepted command line, or for a refusal that a rank other than 0 keeps to
// itself -- and leaves with 1 for a refusal, 0 otherwise.
#include <cstdlib>
#include <iostream>

#include "options.hpp"

int main(int argc, char **argv)
{
    if (argc < 6) { std::cerr << "usage: options_check <devices> <rank_mode> <rank_id> <rank_world> miekki [arguments]" << std::endl; return 2; }
    mkhost::Where where;
    where.devices = (size_t)atol(argv[1]);
    where.rank_mode = atoi(argv[2]) != 0;
    where.rank_id = atoi(argv[3]);
    where.rank_world = atoi(argv[4]);
    mkhost::Options opt;
    mkhost::parse_options(argc - 5, argv + 5, opt);
    mkhost::Checked got;
    const std::string no = mkhost::refusal(opt, where, got);
    std::cout << (got.rank_silenced ? std::string() : no) << std::endl;
    return no.empty() ? 0 : 1;
}
