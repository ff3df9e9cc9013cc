// The command line of `miekki` as data: what was given (Options, parse_options) and the first reason to refuse it
// (refusal), found before a device is touched or a file is written.  Header-only and free of the library: the rules
// are tested without a GPU (tests/helpers/options_check.cpp).
#pragma once
#include <getopt.h>

#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <string>
#include <unordered_set>
#include <vector>

#include "clades.hpp"
#include "hierarchy.hpp"
#include "miekki_hip.h"                        // MK_LIST_CANDIDATES: the header alone
#include "panel.hpp"
#include "reads.hpp"
#include "taxonomy.hpp"
#include "text_file.hpp"

namespace mkhost {

inline void help()
{
    std::cout << "miekki (MI355X build): minhash index for k-mer intersection\n"
            "Input\n"
            "  -i <file>  load a constructed index from disk\n"
            "  -l <file>  construct an index from a list of FASTA files\n"
            "  -M <file>  join the genomes of another index file behind those of -i (same -k -h -f -b; may be repeated; one GPU)\n"
            "  -a <file>  query a FASTA file (one 2-line record per query)\n"
            "  -2 <file>  with -a: the mates of -a's records, record by record (plain or gzip'd): a read pair is ONE query, its k-mers those of each mate alone (one GPU; at most 4,096 k-mers per pair; goes with -n and -P -p -y -Y -U -C -W -D -G; no -e, -A, -X, -S)\n"
            "  -A <file>  query every FASTA file of a list as one sequence\n"
            "  -X         query every genome of the index against the index, from its stored sketch (no FASTA files needed)\n"
            "Output\n"
            "  -o <file>  output file name (out.txt)\n"
            "  -d <file>  dump the index on disk\n"
            "  -n <int>   report at most n genomes per query, 0: every genome above the thresholds (10)\n"
            "  -K <file>  keep only the genomes whose ids the file lists, one per line, in the file's order (before -d and any query)\n"
            "  -F <file>  write the families of the indexed genomes: ids one per line, a blank line between families (a list for -K)\n"
            "  -R <file>  write the representatives of the indexed genomes, earlier ids first: ids one per line (a list for -K; one GPU)\n"
            "  -r <file>  write the clusters around the representatives: -F's layout, a cluster's first id is its representative\n"
            "  -J <list>  with -H and -O: the nested families of the indexed genomes at several thresholds from one pass: 1 to 8 levels, the loosest first, separated by commas, each <min_score> or <min_score>:<min_intersection> (without: 0.5 * -s, -F's; -J 10 is -F's one level) (one GPU)\n"
            "  -H <file>  with -J: the taxonomy of the nested families over the ids of -O's order: <first_id> <last_id> <name> per node (a file for -T)\n"
            "  -O <file>  with -J: the order in which every family of every level is a run of ids: ids one per line (a list for -K)\n"
            "  -P <file>  with -a: no line per read, the profile of the read set: id, best, unique, listed, best_matches per listed genome (one GPU)\n"
            "  -L <file>  with -p: the clades of the indexed genomes, in -F's layout: ids one per line, strictly increasing, a blank line between clades; genomes not named are left out\n"
            "  -p <file>  with -a and -L: no line per read, the profile by clade: clade, first id, members, best, unique, listed, best_matches, hits per listed clade (one GPU; goes with -P, -C, -W, -D, -G)\n"
            "  -T <file>  with -y or -U: the taxonomy of the indexed genomes: a node per line, <first_id> <last_id> [name], nested intervals in preorder; genomes inside no node are left out; -V takes it as well\n"
            "  -y <file>  with -a and -T: no line per read, the reads by lowest common ancestor: node, depth, first id, last id, clade_reads, reads, best_matches, hits, name per node with reads in its subtree (one GPU; goes with -P, -p, -C, -W, -D, -G)\n"
            "  -Y <file>  with -T: every read's node: ordinal, then the node, * for above every node, - for unassigned\n"
            "  -m <int>   with -T: the margin, 0 .. 100 (default 100): the hits within that many percent of a read's best one place it\n"
            "  -U <file>  with -a and -T: no line per read, the distinct covered cells per node of the taxonomy: node, depth, first id, last id, covered cells, held cells, name per node with a covered cell (one GPU; goes with -y -Y -m, -P, -p, -C, -W, -D, -G)\n"
            "  -V <file>  with -a and -T: no line per read, the taxon-specific cells: every held cell belongs to the deepest node that contains all its holders; node, depth, first id, last id, clade_covered, clade_specific, covered, specific, name per node with a covered cell in its subtree (one GPU; goes with -y -Y -m, -U, -P, -p, -E, -C, -W, -D, -G, -2, -q)\n"
            "  -C <file>  with -a: no line per read, the breadth of coverage: id, covered fingerprints, sketch size per covered genome (one GPU; goes with -P)\n"
            "  -W <file>  with -a: no line per read, the winner-takes-all screen: id, cells won, covered fingerprints, sketch size per genome that wins a cell (one GPU; goes with -C, -P)\n"
            "  -S <file>  with -c: a list of read files, one sample per line: the breadth of coverage of every sample, eight samples per pass over the index (one GPU; no -a, -A, -e, -X, -n)\n"
            "  -c <file>  with -S: sample, id, covered fingerprints, sketch size per sample and covered genome\n"
            "  -D <file>  with -a: no line per read, the depth of coverage: id, median and sum of the reads per covered fingerprint, covered fingerprints, sketch size per covered genome (one GPU; goes with -P, -C, -W)\n"
            "  -G <file>  with -a: no line per read, the greedy gather: id, newly explained cells, covered fingerprints, sketch size per picked genome, in pick order; with -D a fifth field, the depth sum of the new cells (one GPU; goes with -P, -C, -W, -D)\n"
            "  -g <int>   with -G: stop when no genome explains at least this many new cells (10)\n"
            "  -E <file>  with -a: no line per read, the abundance by expectation-maximisation: id, reads, unique, shared per genome a read is settled on or shared by; a read that several genomes share is split among them in proportion to what the other reads say (one GPU; goes with -P, -p, -y, -Y, -m, -U, -C, -W, -D, -G)\n"
            "  -I <int>   with -E: the rounds, 1 .. 10000 (50)\n"
            "  -w <int>   with -E: the margin, 0 .. 100 (default 100): the genomes within that many percent of a read's best one share it\n"
            "Performances\n"
            "  -h <int>   use 2^h minimizers per sequence (17)\n"
            "  -k <int>   k-mer size (31)\n"
            "  -q <int>   with -a (and -2) or -S: FASTQ reads are cut at every base whose phred quality is below <int> (0 .. 93): a read's k-mers are those of each stretch of good bases alone, the read stays ONE query (one GPU; at most 4,096 bases per read or pair; every read file must be FASTQ; no -e, -A, -X)\n"
            "  -s <num>   minimal estimated intersection to be reported (200)\n"
            "  -t <int>   host threads that read and parse the input files (8)\n"
            "Advanced usage\n"
            "  -f <int>   fingerprint size: 3 (1-byte) or 11 (2-byte)\n"
            "  -b <int>   2^b bits used for the Bloom filter (33)\n"
            "  -e         exact mode, real intersection is computed on hits\n";
}

struct Options {
    std::string index_file, list_file, query_lines, query_list, output_file = "out.txt", index_dump;   // -i -l -a -A -o -d
    std::string keep_file, families_file, reps_file, clusters_file;                                  // -K -F -R -r
    std::string levels_arg, hierarchy_taxonomy_file, hierarchy_order_file;                           // -J -H -O
    bool levels_given = false;
    std::string profile_file, clades_file, clade_profile_file;                                       // -P -L -p
    std::string taxonomy_file, lca_report_file, lca_reads_file;                                      // -T -y -Y
    std::string cover_file, winners_file, depth_file, gather_file;                                   // -C -W -D -G
    std::string taxon_cover_file;                                                                    // -U
    std::string markers_file;                                                                        // -V
    std::string abundance_file;                                                                      // -E
    std::string panel_list, panel_file, mates_file;                                                  // -S -c -2
    std::vector<std::string> join_files;                                                             // -M, in the order given
    uint64_t H = 17, core_number = 8, kmer_size = 31, bloom_size = 33, fingerprint_size = 3;         // main.cpp:131
    double threshold = 200;
    long nres = 10, min_new = 10, margin = 100, min_qual = -1;                                       // -n -g -m -q
    long rounds = 50, share_margin = 100;                                                            // -I -w
    bool nres_given = false, min_new_given = false, margin_given = false, qual_given = false, threads_given = false;
    bool rounds_given = false, share_margin_given = false;
    bool exact_mode = false, index_queries = false;                                                  // -e -X

    bool want_reps() const { return !reps_file.empty() || !clusters_file.empty(); }
    bool want_hierarchy() const { return levels_given || !hierarchy_taxonomy_file.empty() || !hierarchy_order_file.empty(); }
    // one of the outputs that sum -a's reads on the device instead of listing them
    bool want_profile() const
    {
        return !profile_file.empty() || !cover_file.empty() || !winners_file.empty() || !depth_file.empty() || !gather_file.empty() ||
               !clade_profile_file.empty() || !lca_report_file.empty() || !taxon_cover_file.empty() || !abundance_file.empty() || !markers_file.empty();
    }
};

// -q, -m, -I and -w are read strictly (anything but a whole number: -1, which their ranges refuse); the others as the reference reads its own
inline void parse_options(int argc, char **argv, Options &o)
{
    auto strict = [](const char *arg) { char *rest = nullptr; const long v = strtol(arg, &rest, 10); return rest == arg || *rest ? -1 : v; };
    int c;
    while ((c = getopt(argc, argv, "i:l:a:h:t:f:k:s:b:o:ed:A:n:XK:F:R:r:M:P:C:W:D:G:g:L:p:S:c:T:y:Y:m:2:q:U:E:I:w:J:H:O:V:")) != -1) {
        switch (c) {
        case 'i': o.index_file = optarg; break;
        case 'l': o.list_file = optarg; break;
        case 'a': o.query_lines = optarg; break;
        case 'A': o.query_list = optarg; break;
        case 'o': o.output_file = optarg; break;
        case 'h': o.H = std::stoi(optarg); break;
        case 't': o.core_number = std::stoi(optarg); o.threads_given = true; break;
        case 'k': o.kmer_size = std::stoi(optarg); break;
        case 's': o.threshold = std::stof(optarg); break;
        case 'f': o.fingerprint_size = std::stoi(optarg); break;
        case 'b': o.bloom_size = std::stoi(optarg); break;
        case 'e': o.exact_mode = true; break;
        case 'd': o.index_dump = optarg; break;
        case 'n': o.nres = atol(optarg); o.nres_given = true; break;
        case 'X': o.index_queries = true; break;
        case 'K': o.keep_file = optarg; break;
        case 'F': o.families_file = optarg; break;
        case 'R': o.reps_file = optarg; break;
        case 'r': o.clusters_file = optarg; break;
        case 'J': o.levels_arg = optarg; o.levels_given = true; break;
        case 'H': o.hierarchy_taxonomy_file = optarg; break;
        case 'O': o.hierarchy_order_file = optarg; break;
        case 'M': o.join_files.push_back(optarg); break;
        case 'P': o.profile_file = optarg; break;
        case 'C': o.cover_file = optarg; break;
        case 'W': o.winners_file = optarg; break;
        case 'D': o.depth_file = optarg; break;
        case 'G': o.gather_file = optarg; break;
        case 'g': o.min_new = atol(optarg); o.min_new_given = true; break;
        case 'L': o.clades_file = optarg; break;
        case 'p': o.clade_profile_file = optarg; break;
        case 'S': o.panel_list = optarg; break;
        case 'c': o.panel_file = optarg; break;
        case 'T': o.taxonomy_file = optarg; break;
        case 'y': o.lca_report_file = optarg; break;
        case 'Y': o.lca_reads_file = optarg; break;
        case 'U': o.taxon_cover_file = optarg; break;
        case 'V': o.markers_file = optarg; break;
        case '2': o.mates_file = optarg; break;
        case 'q': o.min_qual = strict(optarg); o.qual_given = true; break;
        case 'm': o.margin = strict(optarg); o.margin_given = true; break;
        case 'E': o.abundance_file = optarg; break;
        case 'I': o.rounds = strict(optarg); o.rounds_given = true; break;
        case 'w': o.share_margin = strict(optarg); o.share_margin_given = true; break;
        }
    }
}

// Where the command runs: the GPUs of the process (every visible one, or MIEKKI_DEVICES) and, when a launcher started one
// process per GPU (torch.distributed.run --no-python sets RANK / WORLD_SIZE / LOCAL_RANK), its place among them.
struct Where {
    size_t devices = 1;
    bool rank_mode = false;
    int rank_id = 0, rank_world = 1, rank_local = 0;
};
inline void rank_from_env(Where &w)
{
    auto env_int = [](const char *a, const char *b, int dflt) { const char *e = getenv(a); if (!e) e = getenv(b); return e ? atoi(e) : dflt; };
    w.rank_world = env_int("MIEKKI_WORLD", "WORLD_SIZE", 1);
    w.rank_id = env_int("MIEKKI_RANK", "RANK", 0);
    w.rank_local = env_int("MIEKKI_LOCAL_RANK", "LOCAL_RANK", w.rank_id);
    w.rank_mode = w.rank_world > 1 || getenv("MIEKKI_WORLD") != nullptr;
}

// What refusal() read on its way through the rules, for main() to go on with
struct Checked {
    std::vector<std::string> panel_samples;     // -S: the files of the list
    std::vector<uint32_t> keep_ids;             // -K
    CladeList clade_list;                       // -L
    Taxonomy taxonomy;                          // -T
    std::vector<mk_level> levels;               // -J, a level without an intersection at 0.5 * the command line's -s
    bool rank_silenced = false;                 // the rules got as far as "rank 0 speaks for all", and this is another rank
};

// the list of -K: one decimal genome id per line, blank lines ignored; false + why for anything else
inline bool parse_keep_list(const std::string &text, const std::string &path, std::vector<uint32_t> &ids, std::string &why)
{
    std::unordered_set<uint32_t> seen;
    size_t line_no = 0;
    for (std::string line : split_lines(text)) {
        ++line_no;
        while (!line.empty() && isspace((unsigned char)line.back())) line.pop_back();
        size_t b = 0;
        while (b < line.size() && isspace((unsigned char)line[b])) ++b;
        line.erase(0, b);
        if (line.empty()) continue;
        const bool digits = line.size() <= 10 && line.find_first_not_of("0123456789") == std::string::npos;
        const unsigned long long v = digits ? strtoull(line.c_str(), nullptr, 10) : 0;
        if (!digits || v > 0xffffffffull) { why = "-K: line " + std::to_string(line_no) + " of " + path + " is not a genome id: " + line; return false; }
        if (!seen.insert((uint32_t)v).second) { why = "-K: genome id " + std::to_string(v) + " is listed twice in " + path; return false; }
        ids.push_back((uint32_t)v);
    }
    if (ids.empty()) { why = "-K: " + path + " lists no genome ids"; return false; }
    return true;
}

// the file a flag names (-K -L -T; an empty path: not given), read and parsed: parse(text, why) is false + why for a bad one
template <class Parse>
std::string file_refusal(const char *flag, const std::string &path, Parse parse)
{
    if (path.empty()) return std::string();
    if (!file_exists(path)) return std::string(flag) + ": cannot read " + path;
    std::string text, why;
    read_text(path, text);
    return parse(text, why) ? std::string() : why;
}

// -q's own rules: the base-quality cut of the reads of -a (and -2) or of -S's samples -- FASTQ files
inline std::string quality_refusal(const Options &o, const Checked &got)
{
    if (o.query_lines.empty() && o.panel_list.empty()) return "-q cuts the reads of a query file at their bad bases: it needs -a or -S";
    if (o.exact_mode || !o.query_list.empty() || o.index_queries) return "-q cuts reads for the approximate mode: it takes no -e, -A or -X";
    if (o.min_qual < 0 || o.min_qual > 93) return "-q takes a phred quality, 0 .. 93";
    std::vector<std::string> files;
    if (!o.query_lines.empty()) files.push_back(o.query_lines);
    if (!o.mates_file.empty()) files.push_back(o.mates_file);
    files.insert(files.end(), got.panel_samples.begin(), got.panel_samples.end());
    for (const std::string &f : files)
        if (file_exists(f) && !file_is_fastq(f)) return "-q needs base qualities: " + f + " is not a FASTQ file (a first byte '@', a third line that starts with '+')";
    return std::string();
}

// The first reason to refuse the command line, or an empty string.  The order of the rules is part of the program's
// behaviour: a command line that breaks two of them is told about the first.
inline std::string refusal(const Options &o, const Where &w, Checked &got)
{
    using std::string;
    // -M: everything that can be refused is refused here, before a device is touched or a file is written
    if (!o.join_files.empty() && o.index_file.empty())
        return o.list_file.empty() ? "-M joins index files to the index that -i loads: it needs -i"
                                   : "-M is not supported with -l: the joined genomes would have no file names (dump the build with -d, then -i ... -M ...)";
    // -2: the mates of -a's records -- a pair is one query of the approximate mode and of every sink over -a's reads
    if (!o.mates_file.empty()) {
        if (o.query_lines.empty()) return "-2 names the mates of the reads of a query file: it needs -a";
        if (o.exact_mode || !o.query_list.empty() || o.index_queries || !o.panel_list.empty()) return "-2 pairs the reads of -a for the approximate mode: it takes no -e, -A, -X or -S";
        if (!file_exists(o.mates_file)) return "-2: cannot read " + o.mates_file;
    }
    // the sinks over the reads of -a likewise (-G's -g below): flag by flag, in this order
    struct SinkFlag { char letter; const string *path; const char *what, *how, *not_hits, *why_one; };
    const SinkFlag sinks[] = {
        {'P', &o.profile_file, "profiles the reads of a query file", "sums the approximate mode's answers over the reads of -a",
         "counts every genome above the thresholds and the best one per read", "a read's best genome is chosen among all of them"},
        {'p', &o.clade_profile_file, "profiles the reads of a query file by clade", "sums the approximate mode's answers over the reads of -a",
         "counts every clade above the thresholds and the best one per read", "a read's best genome is chosen among all of them"},
        {'y', &o.lca_report_file, "places the reads of a query file in a taxonomy", "places the approximate mode's answers for the reads of -a",
         "counts reads per node of the taxonomy, not hits per read", "a read's best genome is chosen among all of them"},
        {'C', &o.cover_file, "screens the reads of a query file", "counts the indexed fingerprints the reads of -a hold",
         "counts covered fingerprints per genome, not hits per read", "the table of seen cells lives on one device"},
        {'W', &o.winners_file, "screens the reads of a query file", "credits the cells the reads of -a hold to the indexed genomes",
         "counts the cells each genome wins, not hits per read", "the table of seen cells lives on one device"},
        {'D', &o.depth_file, "measures the depth of the reads of a query file", "counts the reads of -a that hold each indexed fingerprint",
         "reports a median and a sum per genome, not hits per read", "the table of counters lives on one device"},
        {'G', &o.gather_file, "gathers the genomes that explain the reads of a query file", "picks genomes by the cells the reads of -a hold",
         "reports every pick that explains at least -g new cells, not hits per read", "the table of seen cells lives on one device"},
        {'U', &o.taxon_cover_file, "screens the reads of a query file by the nodes of a taxonomy", "counts the cells the reads of -a hold per node of the taxonomy",
         "counts covered cells per node of the taxonomy, not hits per read", "the table of seen cells lives on one device"},
        {'E', &o.abundance_file, "estimates the abundances from the reads of a query file", "splits the approximate mode's answers for the reads of -a among their genomes",
         "reports reads per genome, not hits per read", "the pool of shared reads lives on one device"},
        {'V', &o.markers_file, "screens the reads of a query file by the cells that belong to one node of a taxonomy", "counts the cells the reads of -a hold per node that owns them",
         "counts covered specific cells per node of the taxonomy, not hits per read", "the table of seen cells lives on one device"},
    };
    for (const SinkFlag &f : sinks) {
        if (f.path->empty()) continue;
        const string flag = string("-") + f.letter + " ";
        if (o.query_lines.empty()) return flag + f.what + ": it needs -a";
        if (o.exact_mode || !o.query_list.empty() || o.index_queries) return flag + f.how + ": it takes no -e, -A or -X";
        if (o.nres_given) return flag + f.not_hits + ": it takes no -n";
    }
    // -S / -c: the samples are the list's files, not -a's reads
    if (o.panel_list.empty() != o.panel_file.empty())
        return o.panel_file.empty() ? "-S screens the samples of a list: it needs -c, the file of their counts" : "-c receives the counts of the samples that -S lists: it needs -S";
    if (!o.panel_list.empty()) {
        if (!o.query_lines.empty() || !o.query_list.empty() || o.exact_mode || o.index_queries) return "-S takes its reads from the files of its list: it takes no -a, -A, -e or -X";
        if (o.nres_given) return "-S counts covered fingerprints per sample and genome, not hits per read: it takes no -n";
        if (!file_exists(o.panel_list)) return "-S: cannot read " + o.panel_list;
        string text;
        read_text(o.panel_list, text);
        panel_list_files(text, got.panel_samples);
        if (got.panel_samples.empty()) return "-S: " + o.panel_list + " names no file";
        for (size_t i = 0; i < got.panel_samples.size(); ++i)
            if (!file_exists(got.panel_samples[i])) return "-S: cannot read sample " + std::to_string(i) + " of " + o.panel_list + ": " + got.panel_samples[i];
    }
    if (o.clade_profile_file.empty() != o.clades_file.empty())
        return o.clades_file.empty() ? "-p profiles the reads by the clades of a file: it needs -L" : "-L names the clades that -p profiles the reads by: it needs -p";
    // -T serves -y, -U or -V (or several of them)
    if (!o.lca_report_file.empty() && o.taxonomy_file.empty()) return "-y reports the reads by the nodes of a taxonomy: it needs -T";
    if (!o.taxonomy_file.empty() && o.lca_report_file.empty() && o.taxon_cover_file.empty() && o.markers_file.empty()) return "-T names the taxonomy that -y reports the reads by: it needs -y";
    if (!o.taxon_cover_file.empty() && o.taxonomy_file.empty()) return "-U counts the covered cells per node of a taxonomy: it needs -T";
    if (!o.markers_file.empty() && o.taxonomy_file.empty()) return "-V credits every cell to the deepest node of a taxonomy that holds it: it needs -T";
    if (!o.lca_reads_file.empty() && o.taxonomy_file.empty()) return "-Y receives every read's node of a taxonomy: it needs -T";
    if (o.margin_given && o.taxonomy_file.empty()) return "-m is the margin of the placement in a taxonomy: it needs -T";
    if (!o.lca_reads_file.empty() && o.lca_report_file.empty()) return "-Y receives every read's node of -y's placement: it needs -y";
    if (o.margin_given && o.lca_report_file.empty()) return "-m is the margin of -y's placement: it needs -y";
    if (o.margin_given && (o.margin < 0 || o.margin > 100)) return "-m takes a percentage, 0 .. 100";
    if (o.min_new_given && o.gather_file.empty()) return "-g is the least a pick of -G has to explain: it needs -G";
    if (o.min_new_given && (o.min_new < 1 || o.min_new > 0xffffffffl)) return "-g takes a number of cells from 1 on: with 0 the picks of -G would not end";
    if (o.rounds_given && o.abundance_file.empty()) return "-I is the number of rounds of -E's estimate: it needs -E";
    if (o.share_margin_given && o.abundance_file.empty()) return "-w is the margin within which genomes share a read of -E's estimate: it needs -E";
    if (o.rounds_given && (o.rounds < 1 || o.rounds > 10000)) return "-I takes a number of rounds, 1 .. 10000";
    if (o.share_margin_given && (o.share_margin < 0 || o.share_margin > 100)) return "-w takes a percentage, 0 .. 100";
    if (o.nres_given && (o.nres < 0 || o.nres >= (long)MK_LIST_CANDIDATES)) return "-n takes a number of genomes per query, or 0 for all of them";
    if (o.nres_given && o.exact_mode) return "-n applies to the approximate mode only: -e reports the reference's hits";
    if (o.index_queries && (o.exact_mode || !o.query_lines.empty() || !o.query_list.empty()))
        return "-X queries the indexed genomes themselves: it takes no query file (-a, -A) and has no exact mode (-e)";
    // -J -H -O: the three go together, and the levels are read here (a level without an intersection: -F's, 0.5 * -s)
    if (o.want_hierarchy()) {
        if (!o.levels_given) return "-H and -O receive the hierarchy of the levels that -J names: they need -J";
        if (o.hierarchy_taxonomy_file.empty()) return "-J lays the nested families out as a taxonomy and an order: it needs -H, the file of the taxonomy";
        if (o.hierarchy_order_file.empty()) return "-J lays the nested families out as a taxonomy and an order: it needs -O, the file of the order";
        string why;
        if (!parse_levels(o.levels_arg, 0.5 * o.threshold, got.levels, why)) return why;
    }
    // one process per GPU?
    if (w.rank_mode && (w.rank_id < 0 || w.rank_id >= w.rank_world)) return "rank " + std::to_string(w.rank_id) + " of " + std::to_string(w.rank_world) + "?";
    got.rank_silenced = w.rank_mode && w.rank_id != 0;                        // rank 0 speaks for all
    // What runs on one GPU of one process only, in the order it is refused in: the flag when it is present, its words, which
    // of the two refusals apply to it (one process per GPU; several GPUs in the process, with the reason).  `first`: rules of
    // the flag's own that come before the two.
    struct OneGpuFlag { bool present; string words; bool ranked, several; const char *why_one; string (*first)(const Options &, const Checked &); };
    std::vector<OneGpuFlag> flags = {
        {o.nres != 10, "-n other than 10 is", true, false, "", nullptr},
        {o.index_queries, "-X is", true, false, "", nullptr},
        {!o.keep_file.empty(), "-K is", true, false, "", nullptr},
        {!o.families_file.empty(), "-F is", true, false, "", nullptr},
        {o.want_reps(), "-R / -r are", true, true, "the rule goes through all ids in order", nullptr},
        {o.want_hierarchy(), "-J -H -O are", true, true, "the forests of all levels live on one device", nullptr},
        {o.qual_given, "-q is", true, true, "a set with qualities lives on one device", quality_refusal},
        {!o.mates_file.empty(), "-2 is", true, true, "a set of pairs lives on one device", nullptr},
    };
    for (const SinkFlag &f : sinks) flags.push_back({!f.path->empty(), string("-") + f.letter + " is", true, true, f.why_one, nullptr});
    flags.push_back({!o.panel_list.empty(), "-S is", true, true, "the table of the samples' cells lives on one device", nullptr});
    flags.push_back({!o.join_files.empty(), "-M is", true, true, "the two indexes are joined on one device", nullptr});
    for (const OneGpuFlag &f : flags) {
        if (!f.present) continue;
        if (f.first) { const string no = f.first(o, got); if (!no.empty()) return no; }
        if (f.ranked && w.rank_mode) return f.words + " not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)";
        if (f.several && w.devices > 1) return f.words + " not supported with several GPUs in the process: " + f.why_one + " (MIEKKI_DEVICES names one)";
    }
    string no = file_refusal("-K", o.keep_file, [&](const string &text, string &why) { return parse_keep_list(text, o.keep_file, got.keep_ids, why); });
    if (no.empty()) no = file_refusal("-L", o.clades_file, [&](const string &text, string &why) { return parse_clades(text, o.clades_file, got.clade_list, why); });
    if (no.empty()) no = file_refusal("-T", o.taxonomy_file, [&](const string &text, string &why) { return parse_taxonomy(text, o.taxonomy_file, got.taxonomy, why); });
    return no;
}

}  // namespace mkhost
