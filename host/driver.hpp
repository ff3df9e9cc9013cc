// The `miekki` binary's driver above the C ABI of include/miekki_hip.h: one Driver per run, its jobs in files of their own
// -- driver_build.cpp (building and editing the index), driver_query.cpp (the query modes), driver_profile.cpp (the sinks
// over -a's reads, -S), driver_exact.cpp (-e) -- and main() in miekki_main.cpp.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "clades.hpp"
#include "fasta_reader.hpp"
#include "miekki_hip.h"
#include "multi_gpu.hpp"
#include "pinned_arena.hpp"
#include "reads.hpp"
#include "rendezvous.hpp"
#include "taxonomy.hpp"
#include "text_file.hpp"

namespace mkhost {

inline std::string int_to_string(uint64_t n)     // utils.cpp:145-157: thousands separators
{
    std::string s = std::to_string(n), out;
    for (size_t i = 0; i < s.size(); ++i) {
        if (i && (s.size() - i) % 3 == 0) out += ',';
        out += s[i];
    }
    return out;
}

inline void die(const std::string &what)
{
    std::cout << what << ": " << mk_last_error() << std::endl;
    exit(1);
}
inline void must(int rc, const std::string &what) { if (rc != MK_OK) die(what); }
inline const char *flush_stream() { std::cout.flush(); return ""; }

// one output line of query_file / query_whole_file (Miekki.cpp:440-444, 503-505)
inline std::string hit_text(const mk_hit *h, uint32_t n)
{
    // to_string(uint) \t to_string(uint) \t to_string(uint(intersection)) \t to_string(double) ";"
    // -- std::to_string(double) is printf's %f -- in one formatting call per hit
    std::string s;
    char buf[96];
    for (uint32_t i = 0; i < n; ++i) {
        const int len = snprintf(buf, sizeof buf, "%u\t%u\t%u\t%f;", h[i].genome, h[i].matches,
                                 (unsigned)h[i].intersection, h[i].jaccard);
        s.append(buf, (size_t)len);
    }
    return s;
}

// `text` as the file a flag names
inline void write_text(const char *flag, const std::string &path, const std::string &text)
{
    std::ofstream f(path.c_str(), std::ios::binary);
    f << text;
    f.close();
    if (!f) { std::cout << flag << ": cannot write " << path << std::endl; exit(1); }
}

// the files a list names: its lines longer than 3 characters (Miekki.cpp:548, 600, 624)
inline std::vector<std::string> read_list(const std::string &path)
{
    std::string text;
    read_text(path, text);
    std::vector<std::string> files;
    for (const std::string &fn : split_lines(text))
        if (fn.size() > 3) files.push_back(fn);
    return files;
}

// One super-batch of a read file, strings and all: the records' head lines and sequences, with -2 the mates' sequences, with
// -q the quality strings of both; and the same as the pointers and lengths the library takes, which point() sets and which
// hold while the strings stay as they are.  With -2 the records are PAIRS: heads, seqs, q, ql are mate 1's.
struct ReadBatch {
    std::vector<std::string> heads, seqs, mates, quals, mate_quals;
    std::vector<const char *> q, mate_q, qual_q, mate_qual_q;
    std::vector<uint64_t> ql, mate_ql;
    void point()
    {
        q.clear(); ql.clear(); mate_q.clear(); mate_ql.clear(); qual_q.clear(); mate_qual_q.clear();
        for (auto &r : seqs) { q.push_back(r.data()); ql.push_back(r.size()); }
        for (auto &r : mates) { mate_q.push_back(r.data()); mate_ql.push_back(r.size()); }
        for (auto &r : quals) qual_q.push_back(r.data());
        for (auto &r : mate_quals) mate_qual_q.push_back(r.data());
    }
};

// The answers to n queries: query i's hits at hits[begin[i]], nhits[i] of them -- filled by a fixed-width call (`width`
// slots per query, the library writes hits and nhits) or from the offsets of a list call
struct Answers {
    std::vector<mk_hit> hits;
    std::vector<uint64_t> begin;
    std::vector<uint32_t> nhits;
    void fixed(size_t n, uint32_t width)
    {
        hits.assign(n * width + 1, mk_hit{});
        nhits.assign(n + 1, 0);
        begin.assign(n + 1, 0);
        for (size_t i = 0; i < n; ++i) begin[i] = i * width;
    }
    void from_offsets(const uint64_t *off, size_t n)                 // (hits: the caller's)
    {
        nhits.assign(n + 1, 0);
        begin.assign(n + 1, 0);
        for (size_t i = 0; i < n; ++i) { begin[i] = off[i]; nhits[i] = (uint32_t)(off[i + 1] - off[i]); }
    }
};

struct Driver {
    DeviceGroup group;                           // one context per GPU, genome shards in list order
    mk_ctx *ctx0() const { return group.ctx(0); }
    unsigned threads = 8;                        // -t: host reader threads
    bool threads_given = false;                  // -t was on the command line: never start more readers than that in total
    uint32_t k = 31, threshold = 200;
    uint32_t nres = 10;                           // -n: genomes reported per query (MK_ALL_RESULTS: every one above the thresholds)
    std::vector<std::string> file_names;         // Miekki.h:59, never persisted
    std::ofstream out;
    std::string mates;                           // -2: the file of the mates of -a's records
    int min_qual = -1;                           // -q: the reads go up with their base qualities and are cut below it on the device
    QualityCount quality;                        // ... and every batch is counted
    void print_quality() { if (min_qual >= 0) std::cout << quality.line((uint32_t)min_qual) << std::endl; }

    // ---- one process per GPU (RCCL): this process builds the rank_id-th contiguous run of the list
    int rank_id = 0, rank_world = 1, rank_local = 0;
    bool forced_rank_mode = false;                // a world of one was asked for explicitly (tests: RCCL on one GPU)
    Rendezvous meet;
    // the GPU of this rank: the LOCAL_RANK-th of MIEKKI_DEVICES when given, else that ordinal
    int rank_device(const std::vector<int> &devices) const { return rank_local < (int)devices.size() ? devices[rank_local] : rank_local; }

    // ---- driver_build.cpp
    // what the shards' builds leave behind (see build_shard's end): readers first, then the arenas their buffers came from
    std::vector<std::unique_ptr<OrderedFastaReader>> kept_readers;
    std::vector<std::shared_ptr<PinnedArena>> kept_arenas;
    std::mutex keep_m;
    ~Driver() { kept_readers.clear(); kept_arenas.clear(); }
    struct ShardBuild { std::string log, error; std::vector<std::string> names; double t_append = 0, t_wait = 0, t_unpack_wait = 0, t_free = 0, t_recycle = 0, t_start = 0, t_total = 0, t_before = 0, t_after = 0, t_lock = 0; size_t slabs = 0; size_t gz_on_device = 0, gz_on_host = 0, from_readers = 0; };
    using MakeCtx = std::function<mk_ctx *(int)>;                   // creates one shard's context on a device ordinal
    void build_shard(mk_ctx *ctx, const std::vector<std::string> &files, unsigned nthreads, bool live, ShardBuild &sb);
    void index_file_of_file(const std::string &list, const std::vector<int> &devices, const MakeCtx &make_ctx);
    void index_file_of_file_ranked(const std::string &list, bool have_list, const std::vector<std::string> &files, const std::vector<int> &devices,
                                   const MakeCtx &make_ctx);
    void report_index();
    mk_comm *make_comm(mk_ctx *ctx);
    void agree(const std::string &mine, const char *what);
    void compress_cold();
    void join_index(const std::string &path, int device);
    void keep_genomes(const std::vector<uint32_t> &ids);
    void finish_index(bool merge_bloom);

    // ---- driver_query.cpp
    static constexpr size_t kSuperBatch = 16384;                 // the records of a super-batch: -Y's room for nodes is as many
    void query_fixed(const std::vector<const char *> &p, const std::vector<uint64_t> &l, uint32_t width, uint32_t min_score, double min_inter, Answers &a);
    void answer(const std::vector<const char *> &p, const std::vector<uint64_t> &l, Answers &a);
    void answer_batch(const ReadBatch &b, Answers &a);
    void answer_indexed(const std::vector<uint32_t> &ids, Answers &a);
    void upload_batch(mk_ctx *ctx, const ReadBatch &b, const char *fail, mk_qset **qs);
    size_t for_read_batches(const std::string &path, const std::function<void(ReadBatch &)> &fn);
    void query_file(const std::string &path);
    void query_file_of_file(const std::string &list);
    void query_index();
    void write_families(const std::string &path);
    void write_representatives(const std::string &reps_path, const std::string &clusters_path);
    void write_hierarchy(const std::string &levels_arg, const std::string &taxonomy_path, const std::string &order_path);

    // ---- driver_profile.cpp
    // What a profile run over -a's reads is asked for, as main() fills it from the flags (an empty path: not that output), and
    // what profile_file adds for the steps: the context, its genomes, the threshold on the intersection, the records read.
    struct ProfileJob {
        std::string reads, tally_path, clade_path, lca_path, nodes_path, cover_path, winners_path, depth_path, gather_path;   // -a -P -p -y -Y -C -W -D -G
        std::string taxon_cover_path;                                         // -U
        std::string markers_path;                                             // -V
        std::string abundance_path;                                           // -E
        uint32_t rounds = 50, share_margin = 100;                             // -I -w
        const CladeList *clades = nullptr;                                    // -L
        const Taxonomy *tax = nullptr;                                        // -T, and the file's name
        std::string tax_name;
        uint32_t margin = 100, min_new = 1;                                   // -m -g
        mk_ctx *ctx = nullptr;
        uint32_t G = 0;
        double min_inter = 0;
        size_t done = 0;
    };
    void profile_file(ProfileJob j);
    void panel_files(const std::vector<std::string> &files, const std::string &out_path);

    // ---- driver_exact.cpp
    struct ExactPending { std::string seq, head; double jaccard, intersection; uint32_t genome; };
    // a genome file as ground_truth_batch sees it: contigs split at '>' lines (Miekki.cpp:805-812)
    struct GenomeContigs { bool exists = false; std::vector<std::string> contigs; };
    GenomeContigs parse_contigs(const std::string &file) const;
    std::vector<std::string> resident;                           // per shard: file whose set B is loaded
    mk_ctx *exact_ctx(const std::vector<ExactPending> &v, size_t &shard);
    bool is_resident(const std::string &file, const std::vector<ExactPending> &v);
    void ground_truth(const std::string &file, const std::vector<ExactPending> &v);
    void ground_truth(const std::string &file, const std::vector<ExactPending> &v, const GenomeContigs &gc);
    bool need_names();
    void exact_collect(const std::vector<std::string> &heads, const std::vector<const std::string *> &seqs, uint32_t nres, uint32_t min_score);
    void query_file_exact(const std::string &path);
    void query_file_of_file_exact(const std::string &list);
};

}  // namespace mkhost
