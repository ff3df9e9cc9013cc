// `miekki` -- drop-in host driver for the -l / -i / -a / -A / -o / -d / -e command
// line of the reference (main.cpp:125-238) on top of libmiekki_hip.so.
//
// Plain C++ above the C ABI of include/miekki_hip.h: flag parsing, FASTA reading,
// batching, output formatting and the index file format stay on the host exactly
// where the reference has them (file drivers Miekki.cpp:426-645, 723-788); every
// sketch / scan / filter / exact-intersection computation is a call into the HIP
// layer.  Differences from the reference, all deliberate:
//   * genome ids follow list order and output follows query order (what the
//     reference does at -t 1) for every -t; -t sets the number of host threads that
//     read and parse input files ahead of the device,
//   * `-i ... -e` reports that genome file names are not stored in an index
//     instead of crashing,
//   * no zlib re-compression of the in-memory columns (main.cpp:198): they live
//     raw in HBM,
//   * where the reference scales with -t threads inside the one process, this one
//     scales over the visible GPUs inside the one process (MIEKKI_DEVICES=0,1,..
//     restricts them): genome shards in list order, one context per GPU
//     (multi_gpu.hpp); ids, hits and files are those of one GPU,
//   * ... or over one PROCESS per GPU with RCCL between them, when a launcher says so:
//         python -m torch.distributed.run --no-python --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1
//             miekki -l genomes.txt -a queries.fa -o out.txt -h 20        (one command line)
//     (RANK / WORLD_SIZE / LOCAL_RANK from the environment, or MIEKKI_RANK / MIEKKI_WORLD / MIEKKI_LOCAL_RANK): rank r
//     indexes the r-th contiguous run of the list on its own GPU, the Bloom filters are folded by one all-reduce,
//     every rank scans all queries against its shard and ONE ncclGather per batch carries the per-query heap
//     entrants to rank 0, which merges them on its GPU and writes the files and the banners (the other ranks stay
//     silent).  -l with -a / -A (and -e); -i and -d need the single-process form.
//   * -X (no argument; not in the reference): every genome of the index against the index, answered from the genomes'
//     stored columns -- what -A over the indexed files themselves prints, without the files (query_index below).
//   * -F <file> (not in the reference): the families the indexed genomes fall into -- connected components of "one is
//     among the other's hits above -X's thresholds" -- computed on the device (write_families below).
//   * -R <file>, -r <file> (not in the reference): greedy representatives over the same links, earlier ids first -- the
//     genomes to keep (a -K list), and the clusters around them (write_representatives below).  One GPU.
//   * -2 <file> with -a (not in the reference; Kraken's --paired): the mates of -a's records, the i-th of one file with the
//     i-th of the other -- a pair is ONE query of the approximate mode and of every flag below over -a's reads: its k-mers
//     are those of each mate alone, mate 1 wins a tie, the Bloom gate is asked for the winner (mk_qset_upload_pairs;
//     host/reads.hpp).  Marks, -Y's ordinals and the summaries count pairs; the head printed is mate 1's.  One GPU.
//   * FASTQ (not in the reference): a read file of -a, -2 or -S whose first byte, after inflation, is '@' and whose third line starts with '+' is read as four-line
//     records, run as their sequences and printed under their head lines, '@' included (host/reads.hpp).  -q <int> with such
//     files (Kraken 2's --minimum-base-quality): the qualities go up with the reads, and the device cuts every read at the
//     bases below <int> -- its k-mers are those of each stretch of good bases alone, the read stays one query
//     (mk_qset_upload_reads); stdout gets one `quality:` line.  One GPU, at most 4,096 bases per read or pair.
//   * -P <file> with -a (not in the reference): the profile of the read set instead of a line per read -- per genome, how many
//     reads list it, list it alone, have it as their best hit -- summed on the device (profile_file below).  One GPU.
//   * -L <file> -p <file> with -a (not in the reference): the same profile by CLADE -- -L groups the indexed genomes in -F's
//     layout, -p gets per clade the reads that list a member (once each), list no other clade, have their best hit in it
//     (mk_qset_run_clade_tally; host/clades.hpp).  Genomes -L does not name are left out of the pass.  Alone or beside -P
//     (one scan serves both) and the flags below.  One GPU.
//   * -T <file> -y <file> [-Y <file>] [-m <margin>] with -a (not in the reference): every read placed in a taxonomy by lowest
//     common ancestor -- -T holds nested intervals of genome ids in preorder, -y gets per node the reads whose hits it is the
//     deepest node to hold, with subtree sums, -Y each read's node (mk_qset_run_lca; host/taxonomy.hpp).  Genomes inside no
//     node are left out of the pass.  Alone or beside the flags around it, with a scan of its own.  One GPU.
//   * -C <file> with -a (not in the reference): breadth of coverage -- per genome, how many of its stored fingerprints the read
//     set's gated sketches hold (mk_qset_run_cover, mk_cover_count; profile_file below).  Alone or beside -P.  One GPU.
//   * -W <file> with -a (not in the reference; Mash screen's -w): the winner-takes-all screen -- every cell the read set marks is
//     credited to ONE genome, the best-contained of its holders, and each genome reports the cells it wins (mk_cover_winners;
//     host/winners.hpp).  One round: the order comes from -C's plain counts.  Alone or beside -C and / or -P.  One GPU.
//   * -S <list> -c <file> (not in the reference): the cover of a cohort -- the list names read files, one sample each; eight
//     samples share one table and one pass over the matrix (mk_qset_run_panel, mk_panel_count; panel_files below; host/panel.hpp).
//     No -a.  One GPU.
//   * -D <file> with -a (not in the reference; Mash screen's median multiplicity): depth of coverage -- per genome, over its
//     stored fingerprints that the read set holds, in how many reads each turns up: the lower median and the sum
//     (mk_qset_run_depth, mk_depth_profile; host/depth.hpp).  Alone or beside -P, -C and -W.  One GPU.
//   * -G <file> with -a, -g <int> (not in the reference; sourmash's gather): the greedy set cover over -C's table -- the genome
//     that explains most of what is still unexplained, its cells struck, and again until no genome explains -g (10) cells: one
//     line per pick, in pick order (mk_cover_gather; host/gather.hpp).  Alone or beside -P, -C, -W and -D.  One GPU.
//   * -M <file> (not in the reference, whose merge_indexes is unfinished): the genomes of another index file behind those of
//     -i, as if both had been built as one list (join_index below).  Repeatable, applied in order; needs -i; one GPU.
#include <getopt.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <future>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "clades.hpp"
#include "taxonomy.hpp"
#include "families.hpp"
#include "fasta_reader.hpp"
#include <zlib.h>

#include "cover.hpp"
#include "depth.hpp"
#include "gather.hpp"
#include "panel.hpp"
#include "winners.hpp"
#include "index_io.hpp"
#include "miekki_hip.h"
#include "multi_gpu.hpp"
#include "profile.hpp"
#include "reads.hpp"
#include "rendezvous.hpp"

using namespace std;

namespace {

string int_to_string(uint64_t n)                 // utils.cpp:145-157: thousands separators
{
    string s = to_string(n), out;
    for (size_t i = 0; i < s.size(); ++i) {
        if (i && (s.size() - i) % 3 == 0) out += ',';
        out += s[i];
    }
    return out;
}

void help()
{
    cout << "miekki (MI355X build): minhash index for k-mer intersection\n"
            "Input\n"
            "  -i <file>  load a constructed index from disk\n"
            "  -l <file>  construct an index from a list of FASTA files\n"
            "  -M <file>  join the genomes of another index file behind those of -i (same -k -h -f -b; may be repeated; one GPU)\n"
            "  -a <file>  query a FASTA file (one 2-line record per query)\n"
            "  -2 <file>  with -a: the mates of -a's records, record by record (plain or gzip'd): a read pair is ONE query, its k-mers those of each mate alone (one GPU; at most 4,096 k-mers per pair; goes with -n and -P -p -y -Y -C -W -D -G; no -e, -A, -X, -S)\n"
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
            "  -P <file>  with -a: no line per read, the profile of the read set: id, best, unique, listed, best_matches per listed genome (one GPU)\n"
            "  -L <file>  with -p: the clades of the indexed genomes, in -F's layout: ids one per line, strictly increasing, a blank line between clades; genomes not named are left out\n"
            "  -p <file>  with -a and -L: no line per read, the profile by clade: clade, first id, members, best, unique, listed, best_matches, hits per listed clade (one GPU; goes with -P, -C, -W, -D, -G)\n"
            "  -T <file>  with -y: the taxonomy of the indexed genomes: a node per line, <first_id> <last_id> [name], nested intervals in preorder; genomes inside no node are left out\n"
            "  -y <file>  with -a and -T: no line per read, the reads by lowest common ancestor: node, depth, first id, last id, clade_reads, reads, best_matches, hits, name per node with reads in its subtree (one GPU; goes with -P, -p, -C, -W, -D, -G)\n"
            "  -Y <file>  with -T: every read's node: ordinal, then the node, * for above every node, - for unassigned\n"
            "  -m <int>   with -T: the margin, 0 .. 100 (default 100): the hits within that many percent of a read's best one place it\n"
            "  -C <file>  with -a: no line per read, the breadth of coverage: id, covered fingerprints, sketch size per covered genome (one GPU; goes with -P)\n"
            "  -W <file>  with -a: no line per read, the winner-takes-all screen: id, cells won, covered fingerprints, sketch size per genome that wins a cell (one GPU; goes with -C, -P)\n"
            "  -S <file>  with -c: a list of read files, one sample per line: the breadth of coverage of every sample, eight samples per pass over the index (one GPU; no -a, -A, -e, -X, -n)\n"
            "  -c <file>  with -S: sample, id, covered fingerprints, sketch size per sample and covered genome\n"
            "  -D <file>  with -a: no line per read, the depth of coverage: id, median and sum of the reads per covered fingerprint, covered fingerprints, sketch size per covered genome (one GPU; goes with -P, -C, -W)\n"
            "  -G <file>  with -a: no line per read, the greedy gather: id, newly explained cells, covered fingerprints, sketch size per picked genome, in pick order; with -D a fifth field, the depth sum of the new cells (one GPU; goes with -P, -C, -W, -D)\n"
            "  -g <int>   with -G: stop when no genome explains at least this many new cells (10)\n"
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

void die(const string &what)
{
    cout << what << ": " << mk_last_error() << endl;
    exit(1);
}

vector<string> split_lines(const string &text)   // getline semantics
{
    vector<string> lines;
    size_t pos = 0;
    while (pos <= text.size()) {
        size_t e = text.find('\n', pos);
        if (e == string::npos) e = text.size();
        lines.emplace_back(text, pos, e - pos);
        pos = e + 1;
    }
    return lines;
}

bool nucleotide_start(const string &s)           // Miekki.cpp:736, 771
{
    return !s.empty() && (s[0] == 'A' || s[0] == 'C' || s[0] == 'G' || s[0] == 'T' || s[0] == 'N');
}

using mkhost::OrderedFastaReader;

// Page-locked memory for the reader pools, in slabs: page-locking is a slow, serialised driver call (a pool of a few
// hundred 2 MB buffers locked one by one costs a visible part of a second at start-up), so buffers are carved out
// of 256 MB slabs and handed back to a free list; the slabs go when the arena goes.  Requests of half a slab or
// more are locked on their own.  Thread-safe (the readers allocate).
class PinnedArena {
public:
    // (a slab is page-locked AHEAD by a thread of the arena's own: sixteen readers that all stand behind one 50 ms driver call
    // whenever a slab runs out -- eleven times while 4,096 gzip'd genomes were read -- lost half a second of inflating)
    explicit PinnedArena(mk_ctx *ctx) : ctx_(ctx), filler_([this] { fill(); }) {}
    ~PinnedArena()
    {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        cv_.notify_all();
        filler_.join();
        if (spare_) mk_host_free(ctx_, spare_);
        for (void *s : slabs_) mk_host_free(ctx_, s);
    }
    void *alloc(size_t bytes)
    {
        bytes = (bytes + 4095) / 4096 * 4096;
        if (bytes >= kSlab / 2) {
            void *p = nullptr;
            if (mk_host_alloc(ctx_, bytes, &p) != MK_OK) return nullptr;
            std::lock_guard<std::mutex> g(m_);
            big_.insert(p);
            return p;
        }
        std::unique_lock<std::mutex> g(m_);
        for (;;) {
            for (size_t i = 0; i < free_.size(); ++i)                // first fit among the blocks handed back
                if (free_[i].second >= bytes) {
                    void *p = free_[i].first;
                    sizes_[p] = free_[i].second;
                    free_.erase(free_.begin() + (long)i);
                    return p;
                }
            if (cur_ && left_ >= bytes) break;
            if (spare_) {                                            // the slab made ahead becomes the current one; the next is asked for
                slabs_.push_back(spare_);
                cur_ = (char *)spare_; left_ = kSlab;
                spare_ = nullptr; want_ = true;
                cv_.notify_all();
                break;
            }
            if (dry_) return nullptr;                                // (no more page-locked memory to be had: the caller takes ordinary memory)
            want_ = true;
            cv_.notify_all();
            const auto t0 = chrono::steady_clock::now();
            const uint64_t seen = released_;
            cv_.wait(g, [&] { return spare_ || dry_ || released_ != seen; });      // (or a block came back that may fit)
            lock_s_ += chrono::duration<double>(chrono::steady_clock::now() - t0).count();
        }
        void *p = cur_;
        cur_ += bytes; left_ -= bytes;
        sizes_[p] = bytes;
        return p;
    }
    void release(void *p)
    {
        std::unique_lock<std::mutex> g(m_);
        if (big_.erase(p)) { g.unlock(); mk_host_free(ctx_, p); return; }
        auto it = sizes_.find(p);
        if (it != sizes_.end()) { free_.emplace_back(p, it->second); sizes_.erase(it); ++released_; g.unlock(); cv_.notify_all(); }
    }
    double lock_s_ = 0;                          // time callers stood waiting for a slab
    size_t n_slabs_ = 0;
private:
    static constexpr size_t kSlab = 256u << 20;
    void fill()                                   // page-locks the next slab whenever the spare one has been taken
    {
        std::unique_lock<std::mutex> g(m_);
        for (;;) {                                // (nothing until somebody asks: an arena that is hardly used locks one slab, on demand)
            cv_.wait(g, [&] { return stop_ || (want_ && !spare_ && !dry_); });
            if (stop_) return;
            want_ = false;
            g.unlock();
            void *s = nullptr;
            const bool ok = mk_host_alloc(ctx_, kSlab, &s) == MK_OK;
            g.lock();
            if (ok) { spare_ = s; ++n_slabs_; } else dry_ = true;
            cv_.notify_all();
        }
    }
    mk_ctx *ctx_;
    std::mutex m_;
    std::condition_variable cv_;
    void *spare_ = nullptr;
    bool want_ = false, dry_ = false, stop_ = false;
    uint64_t released_ = 0;
    vector<void *> slabs_;
    char *cur_ = nullptr;
    size_t left_ = 0;
    vector<std::pair<void *, size_t>> free_;
    std::unordered_map<void *, size_t> sizes_;
    std::unordered_set<void *> big_;
    std::thread filler_;                         // (last: it runs as soon as it exists)
};
void *pinned_alloc(void *arena, size_t bytes) { return ((PinnedArena *)arena)->alloc(bytes); }
void pinned_free(void *arena, void *p) { ((PinnedArena *)arena)->release(p); }

struct Driver {
    mkhost::DeviceGroup group;                   // one context per GPU, genome shards in list order
    mk_ctx *ctx0() const { return group.ctx(0); }
    unsigned threads = 8;                        // -t: host reader threads
    bool threads_given = false;                  // -t was on the command line: never start more readers than that in total
    uint32_t k = 31, threshold = 200;
    uint32_t nres = 10;                           // -n: genomes reported per query (MK_ALL_RESULTS: every one above the thresholds)
    vector<string> file_names;                   // Miekki.h:59, never persisted
    ofstream out;

    // one shard's share of index_file_of_file: files [f0, f1) of the list into ctx, in order.
    // `log` collects what the reference prints meanwhile (one '-' per genome kept, the
    // "Missed file" lines) so that several shards' output can be shown in list order.
    // what the shards' builds leave behind (see build_shard's end): readers first, then the arenas their buffers came from
    vector<std::unique_ptr<OrderedFastaReader>> kept_readers;
    vector<std::shared_ptr<PinnedArena>> kept_arenas;
    std::mutex keep_m;
    ~Driver() { kept_readers.clear(); kept_arenas.clear(); }
    struct ShardBuild { string log, error; vector<string> names; double t_append = 0, t_wait = 0, t_unpack_wait = 0, t_free = 0, t_recycle = 0, t_start = 0, t_total = 0, t_before = 0, t_after = 0, t_lock = 0; size_t slabs = 0; size_t gz_on_device = 0, gz_on_host = 0, from_readers = 0; };
    void build_shard(mk_ctx *ctx, const vector<string> &files, unsigned nthreads, bool live, ShardBuild &sb)
    {
        const double t_enter = chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count();
        // a doubling matrix would hold old and new copy at once: size it for the whole list up front
        if (!files.empty() && mk_reserve(ctx, (uint32_t)files.size()) != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return; }
        // readers parse into pinned buffers, three device batches ahead; the append of one
        // batch returns as soon as its copy is done, so parsing, copying and sketching overlap
        // ... and pack as they parse (2 bits per base, mk_index_append_packed): a quarter of the bytes to buffer and
        // to move over PCIe, and the device skips its own packing pass.
        // gzip'd files -- the reference's normal input (zstr, Miekki.cpp:559) -- arrive as their bytes and are inflated,
        // stripped and appended on the device, a few thousand at a time (a deflate stream is decoded by one lane, so it is
        // the number of streams in flight that makes the rate; MIEKKI_GZ_BATCH sets it, 0 = the readers inflate);
        // whatever the device refuses is inflated here
        // the list goes to the device in units of 512 files, three of them ahead of this thread (fixed: what was measured is in
        // profiles/r6_ingest_gz.txt; a -DMK_TUNE_BUILD binary reads MIEKKI_GZ_BATCH -- 0: the readers inflate everything --,
        // MIEKKI_GZ_IN_FLIGHT, and MIEKKI_GZ_SHARE=1: the readers' own zlib takes a unit whenever three are waiting at the device)
#ifdef MK_TUNE_BUILD
        static const size_t gz_batch = [] { const char *e = getenv("MIEKKI_GZ_BATCH"); return e ? (size_t)std::max(0L, atol(e)) : (size_t)512; }();
        static const size_t gz_in_flight = [] { const char *e = getenv("MIEKKI_GZ_IN_FLIGHT"); return e ? (size_t)std::max(1L, atol(e)) : (size_t)3; }();
        static const bool gz_share = [] { const char *e = getenv("MIEKKI_GZ_SHARE"); return e && atoi(e) != 0; }();
#else
        constexpr size_t gz_batch = 512, gz_in_flight = 3;
        constexpr bool gz_share = false;
#endif
        // A unit's files go to the device as the readers read them (RawSink -> mk_gz_open / mk_gz_stage / mk_gz_put): straight
        // from the page cache into page-locked pieces the library lends, a DMA each, into a batch whose layout the files'
        // sizes fixed -- nothing of a gzip'd file waits in host memory.  A unit the device has no memory for is the readers'.
        // A unit RUNS (mk_gz_run, on a thread of its own) as soon as its last file has been put -- the reader that put it says
        // so -- not when this thread gets round to it: the device inflates the units ahead while the ones before them are
        // being appended.
        struct UnitRun { std::future<int> ran; string error; };
        struct Sink {
            mk_ctx *ctx;
            std::mutex m;
            std::unordered_map<void *, std::shared_ptr<UnitRun>> runs;
            static void *open(void *u, const uint64_t *sizes, uint32_t m, uint64_t *offsets)
            {
                mk_gz_batch *b = nullptr;
                if (mk_gz_open(((Sink *)u)->ctx, sizes, m, &b) != MK_OK) return nullptr;
                if (mk_gz_layout(b, offsets) != MK_OK) { mk_gz_free(b); return nullptr; }
                return b;
            }
            static bool put_span(void *, void *batch, uint32_t first, uint32_t count, const void *data, uint64_t bytes, bool staged)
            {
                return mk_gz_put_span((mk_gz_batch *)batch, first, count, data, bytes, staged ? 1 : 0) == MK_OK;
            }
            static void *stage(void *, void *batch, uint64_t *cap) { return mk_gz_stage((mk_gz_batch *)batch, cap); }
            static bool put(void *, void *batch, uint32_t i, uint64_t at, const void *data, uint64_t bytes, bool staged)
            {
                return mk_gz_put((mk_gz_batch *)batch, i, at, data, bytes, staged ? 1 : 0) == MK_OK;
            }
            static void complete(void *u, void *batch)
            {
                std::shared_ptr<UnitRun> r = std::make_shared<UnitRun>();
                UnitRun *rp = r.get();
                r->ran = std::async(std::launch::async, [rp, batch]() -> int {
                    const int rc = mk_gz_run((mk_gz_batch *)batch);
                    if (rc != MK_OK) rp->error = mk_last_error();
                    return rc;
                });
                std::lock_guard<std::mutex> g(((Sink *)u)->m);
                ((Sink *)u)->runs[batch] = std::move(r);
            }
            std::shared_ptr<UnitRun> take(void *batch)
            {
                std::lock_guard<std::mutex> g(m);
                auto it = runs.find(batch);
                if (it == runs.end()) return nullptr;
                std::shared_ptr<UnitRun> r = std::move(it->second);
                runs.erase(it);
                return r;
            }
            ~Sink() { for (auto &kv : runs) if (kv.second && kv.second->ran.valid()) (void)kv.second->ran.get(); }
        } sink_user;
        sink_user.ctx = ctx;
        mkhost::RawSink sink;
        sink.user = &sink_user; sink.open = Sink::open; sink.stage = Sink::stage; sink.put = Sink::put; sink.put_span = Sink::put_span; sink.complete = Sink::complete;
        // (the arena outlives the reader: declared first.  Both are handed to a thread of their own when the shard is built:
        // giving gigabytes of page-locked memory back takes tenths of a second that nothing has to wait for)
        std::shared_ptr<PinnedArena> arena_p = std::make_shared<PinnedArena>(ctx);
        std::unique_ptr<OrderedFastaReader> reader_p(new OrderedFastaReader(files, nthreads, mkhost::HostAllocator{pinned_alloc, pinned_free, arena_p.get()},
                                                                            std::max<size_t>(3 * 64, gz_in_flight * gz_batch + 64), true, gz_batch != 0,
                                                                            gz_batch, gz_in_flight, gz_batch ? sink : mkhost::RawSink(), gz_share));
        OrderedFastaReader &reader = *reader_p;
        auto now = [] { return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count(); };
        auto show = [&]() { if (live) { cout << sb.log << flush_stream(); sb.log.clear(); } };
        // What has been taken from the readers and waits for its turn, in list order: runs of up to 64 sequences the readers
        // made (packed), and whole UNITS that went to the device -- each run by a thread of its own (mk_gz_run works on a
        // stream of its own; a deflate stream is decoded by few lanes, so it is batches side by side that fill the device).
        // Everything is appended in list order, sixty-four at a time.
        struct Pending {
            vector<OrderedFastaReader::Item> items;
            vector<string> names;
            mk_gz_batch *batch = nullptr;                           // a device unit: its files' bytes are there already
            std::shared_ptr<UnitRun> run;                           // ... and it runs, or has run (the readers started it)
        };
        std::deque<std::unique_ptr<Pending>> pending;
        size_t raw_in_flight = 0, host_waiting = 0;
        std::unique_ptr<Pending> cur;                               // the run being collected
        uint64_t cur_bytes = 0;
        // (whatever way this function is left: no thread of a batch still runs, no batch keeps its blocks)
        struct Cleanup {
            std::deque<std::unique_ptr<Pending>> &pending; std::unique_ptr<Pending> &cur;
            ~Cleanup()
            {
                auto drop = [](Pending *p) { if (!p) return; if (p->run && p->run->ran.valid()) (void)p->run->ran.get(); if (p->batch && p->run) mk_gz_free(p->batch); p->batch = nullptr; };
                for (auto &p : pending) drop(p.get());
                drop(cur.get());
            }
        } cleanup{pending, cur};
        auto close_run = [&]() {
            if (!cur) return;
            if (cur->batch) {
                cur->run = sink_user.take(cur->batch);                // (started when the unit's last file had been put: before its item could be taken)
                ++raw_in_flight;
            } else {
                host_waiting += cur->items.size();
            }
            pending.push_back(std::move(cur));
            cur_bytes = 0;
        };
        auto append_items = [&](const OrderedFastaReader::Item *items, size_t n) {      // sequences the readers made, one call
            const double t0 = now();
            int rc;
            if (items[0].packed) {
                vector<mk_packed_seq> p(n);
                for (size_t i = 0; i < n; ++i) {
                    p[i].codes = items[i].codes; p[i].except = items[i].dirty ? items[i].except : nullptr; p[i].len = items[i].len;
                    memcpy(p[i].head, items[i].head, 32);
                }
                rc = mk_index_append_packed(ctx, p.data(), (uint32_t)n);
            } else {
                vector<const char *> p;
                vector<uint64_t> l;
                for (size_t i = 0; i < n; ++i) { p.push_back(items[i].data); l.push_back(items[i].len); }
                rc = mk_index_append(ctx, p.data(), l.data(), (uint32_t)n);
            }
            if (rc != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return false; }
            sb.t_append += now() - t0;
            return true;
        };
        auto append_host_run = [&](Pending &run) {
            if (!append_items(run.items.data(), run.items.size())) return false;
            sb.names.insert(sb.names.end(), run.names.begin(), run.names.end());
            sb.log.append(run.items.size(), '-');
            host_waiting -= run.items.size();
            sb.from_readers += run.items.size();
            for (auto &s : run.items) reader.recycle(s);
            return true;
        };
        // a file the device did not take (or a whole unit it failed on): read and inflated here, appended in its place
        auto append_from_disk = [&](const string &fn) {
            vector<char> text, scratch, seq;
            if (!mkhost::read_file(fn, text, scratch)) { sb.error = "cannot read " + fn; return false; }
            seq.resize(text.size() + 1);
            seq.resize(mkhost::strip_fasta(text.data(), text.size(), seq.data()));
            ++sb.gz_on_host;
            if (seq.size() < k) return true;
            const char *p = seq.data();
            const uint64_t l = seq.size();
            if (mk_index_append(ctx, &p, &l, 1) != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return false; }
            sb.names.push_back(fn); sb.log += '-';
            return true;
        };
        mk_gz_batch *retired = nullptr;                              // the unit appended last: its text may still be read
        struct Retire { mk_gz_batch *&b; ~Retire() { if (b) mk_gz_free(b); b = nullptr; } } retire{retired};
        auto append_unit = [&](Pending &rb) {
            const double t0 = now();
            const int ran = rb.run ? rb.run->ran.get() : MK_ERR_STATE;
            sb.t_unpack_wait += now() - t0;
            --raw_in_flight;
            // (a batch the device could not run -- no memory for its text, say -- is read again and inflated here, file by
            // file: slower, never wrong; its blocks go back first)
            if (ran != MK_OK) { mk_gz_free(rb.batch); rb.batch = nullptr; }
            vector<uint32_t> which;                                // files of the batch waiting to be appended together
            vector<string> kept;
            bool ok = true;
            auto append = [&]() {
                if (which.empty()) return true;
                const double ta = now();
                if (mk_index_append_gz(ctx, rb.batch, which.data(), (uint32_t)which.size()) != MK_OK) { sb.error = string("index build failed: ") + mk_last_error(); return false; }
                sb.t_append += now() - ta;
                sb.names.insert(sb.names.end(), kept.begin(), kept.end());
                which.clear(); kept.clear();
                return true;
            };
            for (size_t i = 0; i < rb.items.size() && ok; ++i) {
                OrderedFastaReader::Item &it = rb.items[i];
                if (!it.exists) { ok = append(); sb.log += "Missed file: " + rb.names[i] + "\n"; show(); continue; }
                if (it.failed) { ok = append(); if (ok) { sb.error = "cannot read " + rb.names[i]; ok = false; } break; }
                if (!it.raw) {                                     // a file of the unit that came the ordinary way (not gzip'd after all)
                    if (it.len >= k) {
                        ok = append() && append_items(&it, 1);
                        if (ok) { sb.names.push_back(rb.names[i]); sb.log += '-'; ++sb.from_readers; }
                    }
                    continue;
                }
                uint64_t len = 0;
                int32_t st = MK_GZ_INTERNAL;
                if (rb.batch) mk_gz_sequence(rb.batch, it.unit_index, &len, &st);
                if (st != MK_GZ_OK) { ok = append() && append_from_disk(rb.names[i]); continue; }
                if (len >= k) {
                    which.push_back(it.unit_index); kept.push_back(rb.names[i]);
                    sb.log += '-';
                    if (which.size() >= 64) { ok = append(); show(); }
                }
            }
            ok = ok && append();
            // the batch goes when the NEXT unit has been appended (mk_gz_free waits for the strip kernels that read its text:
            // by then they are long done, and this thread has queued the next appends instead of standing here)
            const double tf = now();
            if (retired) mk_gz_free(retired);
            retired = rb.batch;
            rb.batch = nullptr;
            sb.t_free += now() - tf;
            sb.gz_on_device += rb.items.size();
            const double tr = now();
            for (auto &it : rb.items) reader.recycle(it);
            sb.t_recycle += now() - tr;
            reader.raw_consumed(rb.items.size());
            return ok;
        };
        // the front of the queue into the index: everything (all), or whatever is ready now -- and more, waiting for the
        // device, while too much is held back behind it
        auto drain = [&](bool all) {
            while (!pending.empty()) {
                Pending &f = *pending.front();
                if (f.batch && !all && raw_in_flight <= gz_in_flight && host_waiting < 4096 &&
                    f.run && f.run->ran.wait_for(chrono::seconds(0)) != std::future_status::ready) break;
                const bool ok = f.batch ? append_unit(f) : append_host_run(f);
                pending.pop_front();
                show();
                if (!ok) return false;
            }
            return true;
        };
        const double t_loop = now();
        sb.t_before = t_loop - t_enter;
        for (size_t i = 0; i < files.size(); ++i) {
            const string &fn = files[i];
            const double t0 = now();
            OrderedFastaReader::Item item = reader.take(i);
            sb.t_wait += now() - t0;
            if (item.unit_batch) {
                // a file of a device unit, whatever became of it: the unit stays together, in list order, and runs when its
                // last file has been taken (every file has been put then)
                if (cur && cur->batch != (mk_gz_batch *)item.unit_batch) close_run();
                if (!cur) { cur.reset(new Pending()); cur->batch = (mk_gz_batch *)item.unit_batch; }
                cur->items.push_back(item); cur->names.push_back(fn);
                if (item.unit_last) close_run();
                if (!drain(false)) return;
                continue;
            }
            if (!item.exists) { close_run(); if (!drain(true)) return; sb.log += "Missed file: " + fn + "\n"; show(); reader.recycle(item); continue; }
            if (item.failed) { close_run(); (void)drain(true); if (sb.error.empty()) sb.error = "cannot read " + fn; return; }
            if (item.len < k) { reader.recycle(item); continue; }
            if (cur && cur->batch) close_run();
            if (!cur) cur.reset(new Pending());
            cur->items.push_back(item); cur->names.push_back(fn);
            cur_bytes += item.len;
            if (cur->items.size() >= 64 || cur_bytes > (1ull << 30)) close_run();
            if (!drain(false)) return;
        }
        close_run();
        if (!drain(true)) return;
        sb.t_total = now() - t_loop;
        sb.t_lock = arena_p->lock_s_; sb.slabs = arena_p->n_slabs_;
        // the reader's pool and its page-locked arena are kept until the process ends (~Driver), the inflater's blocks until
        // their context goes: giving gigabytes back takes tenths of a second -- inside the index phase when done here, out of the
        // queries' first batches when done beside them (freeing page-locked or device memory stalls the device) -- and a GPU
        // with 288 GB does not miss them
        {
            std::lock_guard<std::mutex> g(keep_m);
            kept_readers.emplace_back(reader_p.release());
            kept_arenas.push_back(std::move(arena_p));
        }
        if (mk_index_size(ctx) != sb.names.size()) sb.error = string("index build failed: ") + mk_last_error();   // settles the last batch
        sb.t_after = now() - t_loop - sb.t_total;
    }

    // ---- Miekki.cpp:540-588.  `make_ctx(device ordinal)` creates one shard's context.
    template <typename MakeCtx>
    void index_file_of_file(const string &list, const vector<int> &devices, MakeCtx make_ctx)
    {
        vector<string> files;
        const bool have_list = mkhost::file_exists(list);
        if (have_list) {
            string text;
            mkhost::read_text(list, text);
            for (const string &fn : split_lines(text))
                if (fn.size() > 3) files.push_back(fn);
        }
        if (rank_world > 1 || forced_rank_mode) { index_file_of_file_ranked(list, have_list, files, devices, make_ctx); return; }
        // genome shards = contiguous runs of the list, one per GPU (never more shards than files)
        const size_t D = std::max<size_t>(1, std::min<size_t>(devices.size(), files.size()));
        vector<mk_ctx *> ctxs;
        for (size_t d = 0; d < D; ++d) ctxs.push_back(make_ctx(devices[d]));
        group.adopt(ctxs);
        if (!have_list) { cout << "Missed file of file: " << list << endl; finish_index(true); return; }
        vector<ShardBuild> sb(D);
        vector<vector<string>> part(D);
        for (size_t d = 0; d < D; ++d) {
            uint64_t b, e;
            mkhost::shard_range(files.size(), (uint32_t)d, (uint32_t)D, b, e);
            part[d].assign(files.begin() + b, files.begin() + e);
        }
        // reader threads per shard: -t as given for one GPU; with several, -t divided by the shards would leave each
        // with a reader or two (the default -t 8 on 8 GPUs: one), far below what a GPU sketches -- so at least eight
        // per shard, as far as the host's cores go
        // ... the CPUs this process may actually use (affinity mask, cgroup quota -- not hardware_concurrency(), which on a
        // 256-thread host with a 16-CPU quota would start 64 readers for 8 shards); an explicit -t is never exceeded in total
        const unsigned hw = mkhost::usable_cpus();
        const unsigned floor_per = threads_given ? 1u : std::min(8u, std::max(1u, hw / (unsigned)D));
        const unsigned per = D == 1 ? std::max(1u, threads) : std::max(1u, std::max(threads / (unsigned)D, floor_per));
        if (D == 1) {
            build_shard(ctxs[0], part[0], per, true, sb[0]);
        } else {                                                   // the shards build side by side
            vector<std::thread> th;
            for (size_t d = 0; d < D; ++d) th.emplace_back([&, d] { build_shard(ctxs[d], part[d], per, false, sb[d]); });
            for (auto &t : th) t.join();
        }
        for (size_t d = 0; d < D; ++d) {                           // what the reference prints, in list order
            cout << sb[d].log;
            if (!sb[d].error.empty()) { cout << endl << sb[d].error << endl; exit(1); }
            file_names.insert(file_names.end(), sb[d].names.begin(), sb[d].names.end());
        }
        cout << endl;
        if (getenv("MIEKKI_VERBOSE"))
            for (size_t d = 0; d < D; ++d)
                cout << "[ingest] shard " << d << ": " << sb[d].names.size() << " genomes, waited for the readers " << sb[d].t_wait
                     << "s, in mk_index_append " << sb[d].t_append << "s, waited for the device's inflater " << sb[d].t_unpack_wait << "s and for its batches' last kernels " << sb[d].t_free << "s (giving the raw files' buffers back " << sb[d].t_recycle << "s, starting batches " << sb[d].t_start << "s, the whole loop " << sb[d].t_total << "s, before it " << sb[d].t_before << "s, after it " << sb[d].t_after << "s; " << sb[d].slabs << " slabs of 256 MB page-locked, readers waited for them " << sb[d].t_lock << "s); gzip'd files inflated on the device " << sb[d].gz_on_device - sb[d].gz_on_host
                     << ", refused by it and inflated here " << sb[d].gz_on_host << "; sequences that came from the readers " << sb[d].from_readers << endl;
        finish_index(true);
        compress_cold();
        cout << "Reference indexed: " << group.total() << endl;
        mk_params p;
        mk_get_params(ctx0(), &p);
        if (p.bloom_log2) cout << "BF size:" << int_to_string(1ull << p.bloom_log2) << endl;
    }

    // ---- one process per GPU (RCCL): this process builds the rank_id-th contiguous run of the list
    int rank_id = 0, rank_world = 1, rank_local = 0;
    bool forced_rank_mode = false;                // a world of one was asked for explicitly (tests: RCCL on one GPU)

    // rank 0 draws the communicator's id and leaves it where the launcher's other children find it (rendezvous.hpp: a file
    // that carries the run's nonce, made exclusively, checked by its readers, gone when everybody has joined)
    mkhost::Rendezvous meet;
    mk_comm *make_comm(mk_ctx *ctx)
    {
        uint8_t id[MK_COMM_ID_BYTES];
        string err;
        if (rank_id == 0) {
            if (mk_comm_unique_id(id) != MK_OK) die("cannot start RCCL");
            static string to_remove;                                   // (whatever ends this process: the file goes)
            to_remove = meet.path;
            atexit([] { if (!to_remove.empty()) unlink(to_remove.c_str()); });
            if (!mkhost::rendezvous_publish(meet, id, sizeof id, err)) { cout << err << endl; exit(1); }
        } else if (!mkhost::rendezvous_fetch(meet, id, sizeof id, 600000, err)) {   // up to ten minutes: rank 0 may still be starting
            cerr << "rank " << rank_id << ": " << err << endl;
            exit(1);
        }
        mk_comm *comm = nullptr;
        if (mk_comm_create(ctx, rank_id, rank_world, id, &comm) != MK_OK) die("cannot create the communicator");
        if (mk_comm_barrier(comm) != MK_OK) die("communicator barrier failed");
        if (rank_id == 0) mkhost::rendezvous_remove(meet);             // everybody has read it
        return comm;
    }

    // Every rank says how it fared (empty = well) before the next collective: if any rank failed, ALL leave here, with the
    // first failure's words on rank 0's stdout -- nobody is left waiting in a collective the failed rank will never enter.
    void agree(const string &mine, const char *what)
    {
        if (!group.ranked()) { if (!mine.empty()) { cout << what << mine << endl; exit(1); } return; }
        vector<string> all;
        string err;
        if (group.all_gather_text(mine, all, err)) { cout << "multi-GPU setup failed: " << err << endl; exit(1); }
        for (const string &e : all)
            if (!e.empty()) { cout << what << e << endl; exit(1); }
    }

    template <typename MakeCtx>
    void index_file_of_file_ranked(const string &list, bool have_list, const vector<string> &files, const vector<int> &devices,
                                   MakeCtx make_ctx)
    {
        // the GPU of this rank: the LOCAL_RANK-th of MIEKKI_DEVICES when given, else that ordinal
        const int device = rank_local < (int)devices.size() ? devices[rank_local] : rank_local;
        mk_ctx *ctx = make_ctx(device);
        group.adopt({ctx});
        group.set_comm(make_comm(ctx));
        if (!have_list) { cout << "Missed file of file: " << list << endl; finish_index(true); return; }
        uint64_t b, e;
        mkhost::shard_range(files.size(), (uint32_t)rank_id, (uint32_t)rank_world, b, e);
        const vector<string> part(files.begin() + b, files.begin() + e);
        ShardBuild sb;
        build_shard(ctx, part, std::max(1u, threads), false, sb);
        // what the reference prints while it indexes, and the names of the genomes that were kept: every rank's, in
        // rank order = list order (an error on any rank ends the run on all of them)
        string err, names;
        for (const string &n : sb.names) { names += n; names += '\n'; }
        vector<string> logs, all_names, errors;
        if (group.all_gather_text(sb.error, errors, err) || group.all_gather_text(sb.log, logs, err) ||
            group.all_gather_text(names, all_names, err)) { cout << "multi-GPU setup failed: " << err << endl; exit(1); }
        for (int r = 0; r < rank_world; ++r) {
            cout << logs[r];
            if (!errors[r].empty()) { cout << endl << errors[r] << endl; exit(1); }
            for (const string &n : split_lines(all_names[r]))
                if (!n.empty()) file_names.push_back(n);
        }
        cout << endl;
        finish_index(true);
        compress_cold();
        cout << "Reference indexed: " << group.total() << endl;
        mk_params p;
        mk_get_params(ctx0(), &p);
        if (p.bloom_log2) cout << "BF size:" << int_to_string(1ull << p.bloom_log2) << endl;
    }

    // INDEX->compress_index(1) of main.cpp:198, for the rows that live in host memory (a collection beyond the GPUs' memory):
    // packed where related genomes sit next to each other in the list, left alone where nothing is to be gained
    void compress_cold()
    {
        for (size_t d = 0; d < group.shards(); ++d) {
            uint64_t raw = 0, packed = 0;
            if (mk_index_compress(group.ctx(d), &raw, &packed) != MK_OK) { cout << "index compression failed: " << mk_last_error() << endl; exit(1); }
            if (raw && getenv("MIEKKI_VERBOSE"))
                cout << "[cold rows] shard " << d << ": " << raw << " bytes in host memory, " << packed << " after packing" << endl;
        }
    }

    // ---- -M: the genomes of another index file behind the index's own (mk_index_extend): the file is loaded into a second
    // context on the same GPU, joined and released.  The joined genomes have no names (an index file stores none).
    void join_index(const string &path, int device)
    {
        string err;
        vector<mk_ctx *> src;
        if (mkhost::load_index(path, {device}, src, err, threads) != 0) { cout << "-M: cannot load " << path << ": " << err << endl; exit(1); }
        const uint32_t n = mk_index_size(src[0]);
        const int rc = group.extend(src[0], err);
        mk_destroy(src[0]);
        if (rc != 0) { cout << "-M: joining " << path << " failed: " << err << endl; exit(1); }
        file_names.clear();
        cout << "Genomes joined: " << n << " from " << path << ", the index holds " << group.total() << endl;
    }

    // ---- -K: the index keeps the genomes `ids` (as -X prints them after -i), in that order (mk_index_select); the file names
    // follow, so that output lines and -e, which reads the genomes' files again, stay right
    void keep_genomes(const vector<uint32_t> &ids)
    {
        const uint32_t G = group.total();
        for (uint32_t id : ids)
            if (id >= G) { cout << "-K: genome id " << id << " is not in the index (it holds " << G << " genomes)" << endl; exit(1); }
        if (group.shards() > 1 && !std::is_sorted(ids.begin(), ids.end())) {
            cout << "-K: a list that is not in ascending order would move genomes between GPUs: run it on one GPU (MIEKKI_DEVICES=0)" << endl;
            exit(1);
        }
        const bool named = file_names.size() == G;
        string err;
        if (group.select(ids.data(), (uint32_t)ids.size(), err) != 0) { cout << "-K: genome selection failed: " << err << endl; exit(1); }
        if (named) {
            vector<string> kept;
            for (uint32_t id : ids) kept.push_back(file_names[id]);
            file_names.swap(kept);
        }
        cout << "Genomes kept: " << group.total() << endl;
    }

    // id bases, the global Bloom filter and the sizes of all genomes on the merging GPU
    void finish_index(bool merge_bloom)
    {
        string err;
        if (group.finish(merge_bloom, err) != 0) { cout << "multi-GPU setup failed: " << err << endl; exit(1); }
    }

    static const char *flush_stream() { cout.flush(); return ""; }

    // one output line of query_file / query_whole_file (Miekki.cpp:440-444, 503-505)
    static string hit_text(const mk_hit *h, uint32_t n)
    {
        // to_string(uint) \t to_string(uint) \t to_string(uint(intersection)) \t to_string(double) ";"
        // -- std::to_string(double) is printf's %f -- in one formatting call per hit
        string s;
        char buf[96];
        for (uint32_t i = 0; i < n; ++i) {
            const int len = snprintf(buf, sizeof buf, "%u\t%u\t%u\t%f;", h[i].genome, h[i].matches,
                                     (unsigned)h[i].intersection, h[i].jaccard);
            s.append(buf, (size_t)len);
        }
        return s;
    }

    void run_query(const vector<const char *> &p, const vector<uint64_t> &l, uint32_t nres, uint32_t min_score,
                   double min_inter, vector<mk_hit> &hits, vector<uint32_t> &nhits)
    {
        hits.assign((size_t)p.size() * nres + 1, mk_hit{});
        nhits.assign(p.size() + 1, 0);
        if (p.empty()) return;
        string err;
        if (group.query(p.data(), l.data(), (uint32_t)p.size(), nres, min_score, min_inter, hits.data(), nhits.data(), err) != 0) {
            cout << "query failed: " << err << endl;
            exit(1);
        }
    }

    // the approximate mode's call, filter_results(query_sequences(batch), nres, 10, 0.5 * threshold) (Miekki.cpp:437, 500): query
    // i's hits at hits[begin[i]], nhits[i] of them -- the reference's ten through the fixed-width path, any other -n as a list
    void run_query_n(const vector<const char *> &p, const vector<uint64_t> &l, vector<mk_hit> &hits, vector<uint64_t> &begin,
                     vector<uint32_t> &nhits)
    {
        begin.assign(p.size() + 1, 0);
        if (nres == 10) {
            run_query(p, l, 10, 10, 0.5 * threshold, hits, nhits);
            for (size_t i = 0; i < p.size(); ++i) begin[i] = i * 10;
            return;
        }
        nhits.assign(p.size() + 1, 0);
        hits.clear();
        if (p.empty()) return;
        string err;
        vector<uint64_t> off;
        if (group.query_list(p.data(), l.data(), (uint32_t)p.size(), nres, 10, 0.5 * threshold, off, hits, err) != 0) {
            cout << "query failed: " << err << endl;
            exit(1);
        }
        for (size_t i = 0; i < p.size(); ++i) { begin[i] = off[i]; nhits[i] = (uint32_t)(off[i + 1] - off[i]); }
    }

    // a batch of for_read_batches as a set on the context -2 and -q run with: reads, pairs (-2: mk_qset_upload_pairs), and with
    // -q either with their base qualities (mk_qset_upload_reads)
    void upload_batch(mk_ctx *ctx, const vector<const char *> &p, const vector<uint64_t> &l, const char *fail, mk_qset **qs)
    {
        const uint32_t n = (uint32_t)p.size();
        if (min_qual >= 0) {
            const bool paired = !mates.empty();
            must(mk_qset_upload_reads(ctx, p.data(), l.data(), qual_q.data(), paired ? mate_q.data() : nullptr, paired ? mate_ql.data() : nullptr,
                                      paired ? mate_qual_q.data() : nullptr, n, (uint32_t)min_qual, qs), "-q: the upload failed");
        } else if (mates.empty()) must(mk_qset_upload(ctx, p.data(), l.data(), n, qs), fail);
        else must(mk_qset_upload_pairs(ctx, p.data(), l.data(), mate_q.data(), mate_ql.data(), n, qs), "-2: the upload failed");
    }

    // the same call for the pairs (p[i], mate_q[i]) of -2, each ONE query (mk_qset_upload_pairs), and for -q's reads or pairs
    // with qualities, on the one context -2 and -q run with
    void run_pairs_n(const vector<const char *> &p, const vector<uint64_t> &l, vector<mk_hit> &hits, vector<uint64_t> &begin,
                     vector<uint32_t> &nhits)
    {
        begin.assign(p.size() + 1, 0);
        nhits.assign(p.size() + 1, 0);
        hits.clear();
        if (p.empty()) return;
        mk_qset *qs = nullptr;
        mk_hitlist *list = nullptr;
        upload_batch(ctx0(), p, l, "-q: the upload failed", &qs);
        must(mk_qset_run_list(ctx0(), qs, nres, 10, 0.5 * threshold, &list), min_qual >= 0 ? "-q: query failed" : "-2: query failed");
        const uint64_t *off = mk_hitlist_offsets(list);
        const mk_hit *h = mk_hitlist_hits(list);
        hits.assign(h, h + off[p.size()]);
        for (size_t i = 0; i < p.size(); ++i) { begin[i] = off[i]; nhits[i] = (uint32_t)(off[i + 1] - off[i]); }
        mk_hitlist_free(list);
        mk_qset_free(ctx0(), qs);
    }

    void run_query(const vector<const string *> &seqs, uint32_t nres, uint32_t min_score, double min_inter,
                   vector<mk_hit> &hits, vector<uint32_t> &nhits)
    {
        vector<const char *> p;
        vector<uint64_t> l;
        for (auto s : seqs) { p.push_back(s->data()); l.push_back(s->size()); }
        run_query(p, l, nres, min_score, min_inter, hits, nhits);
    }

    // strict 2-line records (Miekki.cpp:458-464)
    static void read_records(const string &path, vector<string> &heads, vector<string> &seqs)
    {
        string text;
        mkhost::read_text(path, text);
        vector<string> lines = split_lines(text);
        for (size_t i = 0; i < lines.size(); i += 2) {
            heads.push_back(std::move(lines[i]));
            seqs.push_back(i + 1 < lines.size() ? std::move(lines[i + 1]) : string());
        }
    }

    // the records of a read file, 2-line or FASTQ, and of two files in step (host/reads.hpp)
    using RecordStream = mkhost::RecordStream;
    using PairStream = mkhost::PairStream;
    string mates;                                                // -2: the file of the mates of -a's records
    vector<const char *> mate_q;                                 // mate 2 of the batch that for_read_batches is handing out
    vector<uint64_t> mate_ql;
    // -q: the reads go up with their base qualities (mk_qset_upload_reads) and are cut below min_qual on the device; the
    // batch's quality strings stand here while fn runs, in q's order (mate 2's in mate_qual_q), and every batch is counted
    int min_qual = -1;
    vector<const char *> qual_q, mate_qual_q;
    mkhost::QualityCount quality;
    void print_quality() { if (min_qual >= 0) cout << quality.line((uint32_t)min_qual) << endl; }

    // `text` as the file a flag names
    static void write_text(const char *flag, const string &path, const string &text)
    {
        ofstream f(path.c_str(), std::ios::binary);
        f << text;
        f.close();
        if (!f) { cout << flag << ": cannot write " << path << endl; exit(1); }
    }

    static constexpr size_t kSuperBatch = 16384;                 // the records of a super-batch: -Y's room for nodes is as many

    // The one reader loop over a query file: fn(heads, seqs, q, ql) for its records in super-batches (q, ql: the sequences as
    // the library takes them); the next one is read and split while fn -- the device -- works on this one.  After a batch,
    // one mark per reference batch (345).  Returns the number of records.
    // With -2 the records are PAIRS: heads, seqs, q, ql are mate 1's, and mate 2's sequences of the batch stand in mate_q /
    // mate_ql while fn runs (with_uploaded and run_pairs_n take them from there).
    size_t for_read_batches(const string &path, const std::function<void(vector<string> &, vector<string> &, vector<const char *> &, vector<uint64_t> &)> &fn)
    {
        RecordStream in(path);
        std::unique_ptr<PairStream> pairs(mates.empty() ? nullptr : new PairStream(in, path, mates));
        const bool masked = min_qual >= 0;
        if (masked) (pairs ? pairs->max_bases : in.max_bases) = mkhost::kQualityBasesMax;
        const size_t super = kSuperBatch;
        vector<string> heads, seqs, next_heads, next_seqs, seqs2, next_seqs2, quals, next_quals, quals2, next_quals2;
        size_t done = 0;
        auto read = [&](vector<string> &h, vector<string> &s, vector<string> &s2, vector<string> &x, vector<string> &x2) {
            return pairs ? pairs->next(super, k, h, s, s2, masked ? &x : nullptr, masked ? &x2 : nullptr) : in.next(super, k, h, s, masked ? &x : nullptr);
        };
        // (a mate file that ends early, a pair beyond the short sketch, a FASTQ record that is none, with -q a read beyond the
        // masked sketch: the run ends there, before any sink's file is written)
        auto refuse = [&] {
            const string &why = pairs ? pairs->error : in.error;
            if (!why.empty()) { cout << why << endl; exit(1); }
        };
        bool more = read(heads, seqs, seqs2, quals, quals2);
        refuse();
        while (more) {
            auto ahead = std::async(std::launch::async, [&] { return read(next_heads, next_seqs, next_seqs2, next_quals, next_quals2); });
            vector<const char *> q;
            vector<uint64_t> ql;
            for (auto &r : seqs) { q.push_back(r.data()); ql.push_back(r.size()); }
            mate_q.clear(); mate_ql.clear();
            for (auto &r : seqs2) { mate_q.push_back(r.data()); mate_ql.push_back(r.size()); }
            qual_q.clear(); mate_qual_q.clear();
            if (masked) {
                for (auto &r : quals) qual_q.push_back(r.data());
                for (auto &r : quals2) mate_qual_q.push_back(r.data());
                for (size_t i = 0; i < quals.size(); ++i) {
                    if (pairs) quality.pair(quals[i], quals2[i], k, (uint32_t)min_qual);
                    else quality.read(quals[i], k, (uint32_t)min_qual);
                }
            }
            fn(heads, seqs, q, ql);
            for (size_t i = 0; i < seqs.size(); ++i)
                if (((done + i) % 201) == 0) cout << "-" << flush_stream();
            done += seqs.size();
            more = ahead.get();
            refuse();
            heads.swap(next_heads); seqs.swap(next_seqs); seqs2.swap(next_seqs2); quals.swap(next_quals); quals2.swap(next_quals2);
        }
        return done;
    }

    // ---- Miekki.cpp:426-483
    void query_file(const string &path)
    {
        if (!mkhost::file_exists(path)) { cout << "File problem" << endl; return; }
        vector<mk_hit> hits;
        vector<uint32_t> nhits;
        vector<uint64_t> begin;
        struct WriteJob { vector<string> heads; vector<mk_hit> hits; vector<uint64_t> begin; vector<uint32_t> nhits; size_t n = 0; };
        std::future<void> writer;
        for_read_batches(path, [&](vector<string> &heads, vector<string> &seqs, vector<const char *> &q, vector<uint64_t> &ql) {
            if (mates.empty() && min_qual < 0) run_query_n(q, ql, hits, begin, nhits);
            else run_pairs_n(q, ql, hits, begin, nhits);
            // formatting and writing this batch's lines runs beside the next batch's device work
            // (one writer at a time, in order)
            if (writer.valid()) writer.get();
            auto job = std::make_shared<WriteJob>();
            job->heads.swap(heads); job->hits.swap(hits); job->begin.swap(begin); job->nhits.swap(nhits);
            job->n = seqs.size();
            writer = std::async(std::launch::async, [this, job] {
                string text;
                for (size_t i = 0; i < job->n; ++i) {
                    text += job->heads[i];
                    text += ':';
                    text += hit_text(job->hits.data() + job->begin[i], job->nhits[i]);
                    text += '\n';
                }
                out << text;
            });
        });
        if (writer.valid()) writer.get();
        out << flush;
        print_quality();
    }

    // ---- -P -p -y -C -W -D -G: query_file's reads -- the same records, super-batches and marks, the approximate mode's thresholds --
    // summed on the device instead of listed per read (one context): counters and tables that are reset once, added to by every
    // super-batch's passes, read once at the end.  A super-batch is read and uploaded once for all of them.  Nothing per read
    // comes back but -Y's nodes; the -o file receives nothing.
    // What a profile run over -a's reads is asked for, as main() fills it from the flags (an empty path: not that output), and
    // what profile_file adds for the steps: the context, its genomes, the threshold on the intersection, the records read.
    struct ProfileJob {
        string reads, tally_path, clade_path, lca_path, nodes_path, cover_path, winners_path, depth_path, gather_path;   // -a -P -p -y -Y -C -W -D -G
        const mkhost::CladeList *clades = nullptr;                            // -L
        const mkhost::Taxonomy *tax = nullptr;                                // -T, and the file's name
        string tax_name;
        uint32_t margin = 100, min_new = 1;                                   // -m -g
        mk_ctx *ctx = nullptr;
        uint32_t G = 0;
        double min_inter = 0;
        size_t done = 0;
    };
    static void must(int rc, const string &what) { if (rc != MK_OK) die(what); }
    static void emit(const char *flag, const string &path, const string &text, const string &summary) { write_text(flag, path, text); cout << summary << endl; }

    // The outputs of a profile run, each with its device state and three steps: open (before the reads), run (queues one
    // super-batch's pass), close (the read, the file, the summary line).  A step that fails dies under its own flag.
    struct TallyOut {                                                         // -P
        void *d = nullptr;
        void open(const ProfileJob &j)
        {
            must(mk_dev_alloc(j.ctx, (uint64_t)std::max<uint32_t>(j.G, 1) * sizeof(mk_tally), &d), "-P: no room for the counters");
            must(mk_tally_reset(j.ctx, (mk_tally *)d, j.G), "-P: profile failed");
        }
        void run(const ProfileJob &j, mk_qset *qs) { must(mk_qset_run_tally(j.ctx, qs, 10, j.min_inter, (mk_tally *)d, j.G), "-P: profile failed"); }   // (Miekki.cpp:437's thresholds)
        void close(const ProfileJob &j)
        {
            vector<mk_tally> tally(j.G);
            must(mk_tally_read(j.ctx, (const mk_tally *)d, j.G, tally.data()), "-P: profile failed");
            mk_dev_free(j.ctx, d);
            string text;
            mkhost::ProfileCounts counts;
            mkhost::format_profile(tally.data(), tally.size(), text, counts);
            emit("-P", j.tally_path, text, mkhost::profile_summary(j.done, counts));
        }
    };
    struct CladeOut {                                                         // -L -p
        void *d = nullptr;
        mk_clade_map *map = nullptr;
        uint32_t n = 0;
        void open(const ProfileJob &j)
        {
            vector<uint32_t> ids;                                             // (an id beyond the index is refused here: before the reads are opened)
            string why;
            if (!mkhost::clade_map_of(*j.clades, j.G, ids, why)) { cout << why << endl; exit(1); }
            must(mk_clade_map_create(j.ctx, ids.data(), j.G, &map), "-p: the clade map was refused");
            n = mk_clade_map_size(map);
            must(mk_dev_alloc(j.ctx, (uint64_t)std::max<uint32_t>(n, 1) * sizeof(mk_clade_tally), &d), "-p: no room for the counters");
            must(mk_clade_tally_reset(j.ctx, (mk_clade_tally *)d, n), "-p: profile failed");
        }
        // d_tally: null, or -P's counters, which the same scan then adds to
        void run(const ProfileJob &j, mk_qset *qs, void *d_tally)
        {
            must(mk_qset_run_clade_tally(j.ctx, qs, 10, j.min_inter, map, (mk_clade_tally *)d, n, (mk_tally *)d_tally, j.G), "-p: profile failed");
        }
        void close(const ProfileJob &j)
        {
            vector<mk_clade_tally> ct(n);
            must(mk_clade_tally_read(j.ctx, (const mk_clade_tally *)d, n, ct.data()), "-p: profile failed");
            mk_dev_free(j.ctx, d);
            mk_clade_map_free(j.ctx, map);
            string text;
            mkhost::CladeCounts counts;
            mkhost::format_clade_profile(ct.data(), j.clades->first_id.data(), j.clades->members.data(), ct.size(), text, counts);
            emit("-p", j.clade_path, text, mkhost::clade_summary(j.done, counts));
        }
    };
    struct LcaOut {                                                           // -T -y -Y -m
        void *d = nullptr, *d_node = nullptr;                                 // the counters; with -Y, room for a super-batch's nodes
        mk_taxonomy *taxonomy = nullptr;
        uint32_t n_slots = 0;
        string node_text;
        vector<uint32_t> nodes;
        size_t run_before = 0;                                                // the records of the super-batches before this one
        void open(const ProfileJob &j)
        {
            string why;                                                       // (an id beyond the index is refused here: before the reads are opened)
            if (!mkhost::taxonomy_fits(*j.tax, j.tax_name, j.G, why)) { cout << why << endl; exit(1); }
            n_slots = (uint32_t)j.tax->lo.size() + 1;
            must(mk_taxonomy_create(j.ctx, j.tax->lo.data(), j.tax->hi.data(), n_slots - 1, j.G, &taxonomy), "-T: the taxonomy was refused");
            must(mk_dev_alloc(j.ctx, (uint64_t)n_slots * sizeof(mk_lca_tally), &d), "-y: no room for the counters");
            must(mk_lca_tally_reset(j.ctx, (mk_lca_tally *)d, n_slots), "-y: lca failed");
            if (!j.nodes_path.empty()) must(mk_dev_alloc(j.ctx, kSuperBatch * sizeof(uint32_t), &d_node), "-Y: no room for the nodes");
        }
        // a pass of its own; with -Y the batch's n nodes come back after it, the only thing per read that does
        void run(const ProfileJob &j, mk_qset *qs, size_t n)
        {
            if (d_node && n > kSuperBatch) die("-Y: a super-batch beyond the nodes' room");
            must(mk_qset_run_lca(j.ctx, qs, 10, j.min_inter, j.margin, taxonomy, (mk_lca_tally *)d, n_slots, (uint32_t *)d_node), "-y: lca failed");
            if (d_node && n) {
                nodes.resize(n);
                must(mk_dev_download(j.ctx, nodes.data(), d_node, n * sizeof(uint32_t)), "-Y: lca failed");
                mkhost::format_lca_reads(nodes.data(), nodes.size(), run_before, node_text);
            }
            run_before += n;
        }
        void close(const ProfileJob &j)
        {
            vector<mk_lca_tally> lt(n_slots);
            must(mk_lca_tally_read(j.ctx, (const mk_lca_tally *)d, n_slots, lt.data()), "-y: lca failed");
            mk_dev_free(j.ctx, d);
            if (d_node) mk_dev_free(j.ctx, d_node);
            mk_taxonomy_free(j.ctx, taxonomy);
            string text;
            mkhost::LcaCounts counts;
            mkhost::format_lca_report(lt.data(), *j.tax, text, counts);
            write_text("-y", j.lca_path, text);
            if (d_node) write_text("-Y", j.nodes_path, node_text);
            cout << mkhost::lca_summary(j.done, counts, j.margin) << endl;
        }
    };
    struct SeenOut {                                                          // the table of seen cells: -C, -W and -G read it
        void *d = nullptr;
        string flag;                                                          // the first of -C -W -G that was given
        void open(const ProfileJob &j)
        {
            flag = !j.cover_path.empty() ? "-C" : !j.winners_path.empty() ? "-W" : "-G";
            must(mk_dev_alloc(j.ctx, mk_cover_bytes(j.ctx), &d), flag + ": no room for the table");
            must(mk_cover_reset(j.ctx, (uint32_t *)d), flag + ": cover failed");
        }
        void run(const ProfileJob &j, mk_qset *qs) { must(mk_qset_run_cover(j.ctx, qs, (uint32_t *)d), flag + ": cover failed"); }
        // -C and -W: with both, the count pass runs once and serves both files.  The table stays for -G.
        void close(const ProfileJob &j)
        {
            const bool want_winners = !j.winners_path.empty();
            vector<uint32_t> covered(j.G), won(j.G), sketch;
            uint64_t cells = 0, claimed = 0;
            mk_params p;
            const int rc = want_winners ? mk_cover_winners(j.ctx, (const uint32_t *)d, covered.data(), won.data(), &cells, &claimed)
                                        : mk_cover_count(j.ctx, (const uint32_t *)d, covered.data(), &cells);
            if (rc != MK_OK || !index_sizes(j.ctx, j.G, p, sketch)) die(flag + ": cover failed");
            if (j.gather_path.empty()) mk_dev_free(j.ctx, d);
            string text;
            if (!j.cover_path.empty()) {
                const uint64_t genomes = mkhost::format_cover(covered.data(), sketch.data(), covered.size(), text);
                emit("-C", j.cover_path, text, mkhost::cover_summary(j.done, cells, p.h, p.fp_bits, genomes));
                text.clear();
            }
            if (want_winners) {
                const uint64_t genomes = mkhost::format_winners(won.data(), covered.data(), sketch.data(), j.G, text);
                emit("-W", j.winners_path, text, mkhost::winners_summary(j.done, claimed, cells, genomes));
            }
        }
        // -G, after everything else: the greedy rounds over a copy of the table, with -D's table (d_mult, or null) for the fifth
        // field; both tables go here
        void gather(const ProfileJob &j, void *d_mult)
        {
            vector<mk_pick> picks(j.G);
            uint32_t n_picks = 0;
            uint64_t cells = 0, explained = 0;
            must(mk_cover_gather(j.ctx, (const uint32_t *)d, (const uint8_t *)d_mult, j.min_new, 0, picks.data(), &n_picks, &cells, &explained), "-G: gather failed");
            mk_dev_free(j.ctx, d);
            if (d_mult) mk_dev_free(j.ctx, d_mult);
            string text;
            mkhost::format_gather(picks.data(), n_picks, d_mult != nullptr, text);
            emit("-G", j.gather_path, text, mkhost::gather_summary(j.done, explained, cells, n_picks, j.min_new));
        }
    };
    struct DepthOut {                                                         // -D
        void *d = nullptr;
        void open(const ProfileJob &j)
        {
            must(mk_dev_alloc(j.ctx, mk_depth_bytes(j.ctx), &d), "-D: no room for the table");
            must(mk_depth_reset(j.ctx, (uint8_t *)d), "-D: depth failed");
        }
        void run(const ProfileJob &j, mk_qset *qs) { must(mk_qset_run_depth(j.ctx, qs, (uint8_t *)d), "-D: depth failed"); }
        void close(const ProfileJob &j)                                       // (the table stays for -G)
        {
            vector<mk_depth> depth(j.G);
            vector<uint32_t> sketch;
            uint64_t cells = 0, saturated = 0;
            mk_params p;
            if (mk_depth_profile(j.ctx, (const uint8_t *)d, depth.data(), &cells, &saturated) != MK_OK || !index_sizes(j.ctx, j.G, p, sketch)) die("-D: depth failed");
            if (j.gather_path.empty()) mk_dev_free(j.ctx, d);
            string text;
            const uint64_t genomes = mkhost::format_depth(depth.data(), sketch.data(), j.G, text);
            emit("-D", j.depth_path, text, mkhost::depth_summary(j.done, cells, saturated, p.h, p.fp_bits, genomes));
        }
    };

    // the parameters and the sketch sizes that the cover, winners, depth and panel files are formatted with
    static bool index_sizes(mk_ctx *ctx, uint32_t G, mk_params &p, vector<uint32_t> &sketch)
    {
        vector<uint64_t> sizes(G);
        sketch.resize(G);
        return mk_get_params(ctx, &p) == MK_OK && (!G || mk_index_export_sizes(ctx, sizes.data(), sketch.data()) == MK_OK);
    }

    // One super-batch as a set on the device for fn(qs), whose steps die under their own flags, and freed after it -- which
    // waits for the passes fn queued.  The upload is a step too: `fail` is what it dies with.
    template <class Fn>
    void with_uploaded(mk_ctx *ctx, vector<const char *> &q, vector<uint64_t> &ql, const char *fail, Fn fn)
    {
        mk_qset *qs = nullptr;
        // (-2: the batch's pairs as one query each, -q: cut at their bad bases -- every pass over the set is what it is for reads)
        upload_batch(ctx, q, ql, fail, &qs);
        fn(qs);
        mk_qset_free(ctx, qs);
    }

    // The fixed sequence over the outputs: open, per super-batch the passes in the order tally or clades, cover, depth, lca --
    // one upload serves them all --, then the closes in the order of the summary lines.
    void profile_file(ProfileJob j)
    {
        j.ctx = ctx0(); j.G = group.total(); j.min_inter = 0.5 * threshold;
        const bool want_tally = !j.tally_path.empty(), want_clades = !j.clade_path.empty(), want_lca = !j.lca_path.empty();
        const bool want_gather = !j.gather_path.empty(), want_depth = !j.depth_path.empty();
        const bool want_readers = !j.cover_path.empty() || !j.winners_path.empty(), want_seen = want_readers || want_gather;
        TallyOut tally;
        CladeOut clades;
        LcaOut lca;
        SeenOut seen;
        DepthOut depth;
        if (want_clades) clades.open(j);
        if (want_lca) lca.open(j);
        if (!mkhost::file_exists(j.reads)) { cout << "File problem" << endl; return; }
        if (want_tally) tally.open(j);
        if (want_seen) seen.open(j);
        if (want_depth) depth.open(j);
        j.done = for_read_batches(j.reads, [&](vector<string> &, vector<string> &, vector<const char *> &q, vector<uint64_t> &ql) {
            with_uploaded(j.ctx, q, ql, "-a: the upload failed", [&](mk_qset *qs) {   // (every pass is queued)
                if (want_clades) clades.run(j, qs, tally.d);                  // (with -P: its counters from the same scan)
                else if (want_tally) tally.run(j, qs);
                if (want_seen) seen.run(j, qs);
                if (want_depth) depth.run(j, qs);
                if (want_lca) lca.run(j, qs, q.size());
            });
        });
        print_quality();
        if (want_tally) tally.close(j);
        if (want_clades) clades.close(j);
        if (want_lca) lca.close(j);
        if (want_readers) seen.close(j);
        if (want_depth) depth.close(j);
        if (want_gather) seen.gather(j, depth.d);
    }

    // ---- -S / -c: every listed file is a sample, read as -a reads one; the samples go in groups of eight through one table of
    // (partition, value) bytes -- reset, every file's super-batches marked into its slot's bit (mk_qset_run_panel), one pass over
    // the matrix for the group (mk_panel_count).  The -o file receives nothing.
    void panel_files(const vector<string> &files, const string &out_path)
    {
        mk_ctx *ctx = ctx0();
        const uint32_t G = group.total();
        void *d_panel = nullptr;
        mk_params p;
        vector<uint32_t> sketch;
        if (!index_sizes(ctx, G, p, sketch)) die("-S: panel failed");
        if (mk_dev_alloc(ctx, mk_panel_bytes(ctx), &d_panel) != MK_OK) die("-S: no room for the table");
        string text;
        for (size_t s0 = 0; s0 < files.size(); s0 += MK_PANEL_SLOTS) {
            const uint32_t n = (uint32_t)std::min<size_t>(MK_PANEL_SLOTS, files.size() - s0);
            if (mk_panel_reset(ctx, (uint8_t *)d_panel) != MK_OK) die("-S: panel failed");
            vector<size_t> done(n);
            for (uint32_t slot = 0; slot < n; ++slot)
                done[slot] = for_read_batches(files[s0 + slot], [&](vector<string> &, vector<string> &, vector<const char *> &q, vector<uint64_t> &ql) {
                    with_uploaded(ctx, q, ql, "-S: panel failed", [&](mk_qset *qs) {
                        if (mk_qset_run_panel(ctx, qs, slot, (uint8_t *)d_panel) != MK_OK) die("-S: panel failed");             // (queued)
                    });
                });
            vector<uint32_t> covered((size_t)n * G);
            vector<uint64_t> cells(n);
            if (mk_panel_count(ctx, (const uint8_t *)d_panel, n, covered.data(), cells.data()) != MK_OK) die("-S: panel failed");
            for (uint32_t slot = 0; slot < n; ++slot) {
                const uint64_t genomes = mkhost::format_panel(s0 + slot, covered.data() + (size_t)slot * G, sketch.data(), G, text);
                cout << mkhost::panel_sample_summary(s0 + slot, done[slot], cells[slot], p.h, p.fp_bits, genomes) << endl;
            }
        }
        mk_dev_free(ctx, d_panel);
        write_text("-c", out_path, text);
        print_quality();
        cout << mkhost::panel_summary(files.size(), MK_PANEL_SLOTS) << endl;
    }

    // ---- Miekki.cpp:592-612, 487-514
    void query_file_of_file(const string &list)
    {
        if (!mkhost::file_exists(list)) { cout << "Missed file of file: " << list << endl; return; }
        string text;
        mkhost::read_text(list, text);
        vector<string> files;
        for (const string &fn : split_lines(text))
            if (fn.size() > 3) files.push_back(fn);
        // readers parse into pinned buffers, two batches ahead: the upload of a batch is a DMA
        // straight out of them
        PinnedArena arena(ctx0());
        OrderedFastaReader reader(files, threads, mkhost::HostAllocator{pinned_alloc, pinned_free, &arena}, 2 * 64);
        // whole files are queried 64 at a time: the dense kernel scores sixteen per wave and lets the four waves of a workgroup
        // walk the same rows together (the later sets find them in the Infinity Cache): 80 ms for 64 queries against 100,000 genomes, 44 ms for 32; output stays
        // in list order
        vector<string> names;
        vector<OrderedFastaReader::Item> refs;
        uint64_t bytes = 0;
        auto flush = [&]() {
            if (refs.empty()) return;
            vector<const char *> p;
            vector<uint64_t> l;
            for (auto &r : refs) { p.push_back(r.data); l.push_back(r.len); }
            vector<mk_hit> hits;
            vector<uint64_t> begin;
            vector<uint32_t> nhits;
            run_query_n(p, l, hits, begin, nhits);
            for (size_t i = 0; i < refs.size(); ++i)
                if (nhits[i]) out << names[i] << ":" << hit_text(hits.data() + begin[i], nhits[i]) << "\n";   // 506-511
            out << std::flush;
            for (auto &r : refs) reader.recycle(r);
            names.clear(); refs.clear(); bytes = 0;
        };
        for (size_t i = 0; i < files.size(); ++i) {
            OrderedFastaReader::Item item = reader.take(i);
            if (!item.exists) {
                cout << "File problem" << endl;
                reader.recycle(item);
            } else if (item.failed) {
                cout << "cannot read " << files[i] << endl;
                exit(1);
            } else if (item.len >= k) {
                bytes += item.len;
                names.push_back(files[i]); refs.push_back(item);
                if (refs.size() >= 64 || bytes > (1ull << 30)) flush();
            } else {
                reader.recycle(item);
            }
            cout << "-" << flush_stream();
        }
        flush();
    }

    // ---- -X: query_whole_file (Miekki.cpp:487-514) for every INDEXED genome, without its file: the genome's stored column
    // is the gated sketch query_sequence would compute for its sequence (same minhash_sketch_partition, 281 / 320; the
    // Bloom gate passes every active partition of an inserted genome, 295-299 + 135-146).  In id order, 64 genomes at a
    // time; a line starts with the genome's file name when this run built the index from a list, else with its id.
    void query_index()
    {
        const uint32_t G = group.total();
        const bool named = G && file_names.size() == G;
        vector<uint32_t> ids;
        vector<mk_hit> hits;
        vector<uint32_t> nhits;
        vector<uint64_t> begin;
        string err;
        for (uint32_t g0 = 0; g0 < G; g0 += 64) {
            const uint32_t m = std::min<uint32_t>(64, G - g0);
            ids.resize(m);
            for (uint32_t i = 0; i < m; ++i) ids[i] = g0 + i;
            begin.assign(m + 1, 0);
            int rc;
            if (nres == 10) {
                hits.assign((size_t)m * 10 + 1, mk_hit{});
                nhits.assign(m + 1, 0);
                rc = group.query_indexed(ids.data(), m, 10, 10, 0.5 * threshold, hits.data(), nhits.data(), err);   // 500
                for (uint32_t i = 0; i < m; ++i) begin[i] = (uint64_t)i * 10;
            } else {
                rc = group.query_indexed_list(ids.data(), m, nres, 10, 0.5 * threshold, begin, hits, err);
                nhits.assign(m + 1, 0);
                for (uint32_t i = 0; rc == 0 && i < m; ++i) nhits[i] = (uint32_t)(begin[i + 1] - begin[i]);
            }
            if (rc != 0) { cout << "query failed: " << err << endl; exit(1); }
            for (uint32_t i = 0; i < m; ++i) {
                if (nhits[i]) {                                                                                     // 506-511
                    if (named) out << file_names[g0 + i]; else out << g0 + i;
                    out << ":" << hit_text(hits.data() + begin[i], nhits[i]) << "\n";
                }
                cout << "-" << flush_stream();
            }
            out << std::flush;
        }
    }

    // ---- -F: the families of the indexed genomes at -X's thresholds (mk_index_families; several GPUs: a forest per shard,
    // folded on the first), written as a list -K takes: families by ascending label, members ascending, a blank line between
    void write_families(const string &path)
    {
        vector<uint32_t> labels;
        string err, text;
        if (group.families(10, 0.5 * threshold, labels, err) != 0) { cout << "-F: families failed: " << err << endl; exit(1); }
        mkhost::FamilyCounts counts;
        if (!mkhost::format_families(labels.data(), labels.size(), text, counts, err)) { cout << "-F: " << err << endl; exit(1); }
        write_text("-F", path, text);
        cout << mkhost::family_summary(counts) << endl;
    }

    // ---- -R / -r: greedy representatives in id order at -X's thresholds (mk_index_representatives; one context).  -R: the
    // representatives ascending, a list -K takes; -r: rep[] has the shape of family labels, so the clusters are written as -F
    // writes families -- by ascending representative, which is a cluster's first line
    void write_representatives(const string &reps_path, const string &clusters_path)
    {
        vector<uint32_t> rep;
        string err, text;
        if (group.representatives(10, 0.5 * threshold, rep, err) != 0) { cout << "-R / -r: representatives failed: " << err << endl; exit(1); }
        mkhost::FamilyCounts counts;
        if (!mkhost::format_families(rep.data(), rep.size(), text, counts, err)) { cout << "-R / -r: " << err << endl; exit(1); }
        if (!reps_path.empty()) {
            string list;
            for (size_t j = 0; j < rep.size(); ++j)
                if (rep[j] == j) { list += to_string(j); list += '\n'; }
            write_text("-R", reps_path, list);
        }
        if (!clusters_path.empty()) write_text("-r", clusters_path, text);
        cout << "representatives: " << counts.families << " of " << rep.size() << ", largest cluster " << counts.largest << endl;
    }

    // ---- exact mode -------------------------------------------------------------
    struct Pending { string seq, head; double jaccard, intersection; uint32_t genome; };

    // a genome file as ground_truth_batch sees it: contigs split at '>' lines (Miekki.cpp:805-812),
    // walked line by line over the raw text.  Callable from a helper thread.
    struct GenomeContigs { bool exists = false; vector<string> contigs; };
    GenomeContigs parse_contigs(const string &file) const
    {
        GenomeContigs gc;
        gc.exists = mkhost::file_exists(file);
        if (!gc.exists) return gc;
        vector<char> text, scratch;
        mkhost::read_file(file, text, scratch);
        string ref;
        ref.reserve(text.size());
        const char *pos = text.data(), *const end = text.data() + text.size();
        while (pos <= end) {                                                     // getline semantics
            const char *e = pos < end ? (const char *)memchr(pos, '\n', (size_t)(end - pos)) : nullptr;
            if (!e) e = end;
            if (e != pos && *pos == '>') {
                if (ref.size() >= k) { gc.contigs.push_back(std::move(ref)); ref = string(); }   // short contigs leak (806-812)
            } else {
                ref.append(pos, (size_t)(e - pos));
            }
            pos = e + 1;
        }
        if (ref.size() >= k) gc.contigs.push_back(std::move(ref));
        return gc;
    }

    // ground_truth_batch (Miekki.cpp:792-859) for all pending queries of one genome file.  The
    // reference rebuilds the file's k-mer set at every call (~7 s); here the set stays resident on
    // the GPU that verified the file last, so a file whose queries are flushed in several batches
    // (the flush-at-100 rule) is read, split and hashed once.
    vector<string> resident;                                     // per shard: file whose set B is loaded
    mk_ctx *exact_ctx(const vector<Pending> &v, size_t &shard)
    {
        // K7 runs on the GPU that owns the genome (any would do: the sets come from the file itself)
        shard = v.empty() || group.ranked() ? 0 : group.owner(v[0].genome);
        if (resident.size() != group.shards()) resident.assign(group.shards(), string());
        return group.ctx(shard);
    }
    bool is_resident(const string &file, const vector<Pending> &v)
    {
        size_t shard;
        exact_ctx(v, shard);
        return !file.empty() && resident[shard] == file;
    }

    void ground_truth(const string &file, const vector<Pending> &v)
    {
        if (is_resident(file, v)) ground_truth(file, v, GenomeContigs{});
        else ground_truth(file, v, parse_contigs(file));
    }

    void ground_truth(const string &file, const vector<Pending> &v, const GenomeContigs &gc)
    {
        size_t shard;
        mk_ctx *ctx = exact_ctx(v, shard);
        if (resident[shard] != file) {
            if (!gc.exists) { cout << "File problem: " << file << endl; return; }
            vector<const char *> cp;
            vector<uint64_t> cl;
            for (auto &c : gc.contigs) { cp.push_back(c.data()); cl.push_back(c.size()); }
            resident[shard].clear();
            if (mk_exact_load_genome(ctx, cp.data(), cl.data(), (uint32_t)gc.contigs.size()) != MK_OK) die("exact mode failed");
            resident[shard] = file;
        }
        vector<const char *> qp;
        vector<uint64_t> ql;
        for (auto &q : v) { qp.push_back(q.seq.data()); ql.push_back(q.seq.size()); }
        vector<uint64_t> inter(v.size()), uni(v.size());
        if (mk_exact_query(ctx, qp.data(), ql.data(), (uint32_t)v.size(), inter.data(), uni.data()) != MK_OK)
            die("exact mode failed");
        for (size_t i = 0; i < v.size(); ++i) {
            if (!inter[i]) continue;                                             // 843
            const double real_jax = (double)inter[i] / (double)uni[i];
            out << real_jax << "\t" << v[i].jaccard << "\t" << (double)inter[i] << "\t" << v[i].intersection
                << "\t" << v[i].head << "\t" << file << "\n";                    // 853
        }
    }

    bool need_names()
    {
        if (file_names.size() == group.total()) return true;
        cout << "exact mode needs the genome files of the index: build it with -l in the same run "
                "(file names are not stored in an index file)" << endl;
        return false;
    }

    void exact_collect(const vector<string> &heads, const vector<const string *> &seqs, uint32_t nres,
                       uint32_t min_score)
    {
        vector<mk_hit> hits;
        vector<uint32_t> nhits;
        run_query(seqs, nres, min_score, (double)threshold, hits, nhits);
        if (!group.root()) return;                                   // (one process per GPU: rank 0 verifies and writes)
        // Same container, same insertion sequence and the same flush-at-100 rule as the
        // reference (Miekki.cpp:728-754, 779-785): with the same libstdc++ the lines of the
        // output file then come out in the reference's order, not just as the same set.
        unordered_map<string, vector<Pending>> batch;
        for (size_t q = 0; q < seqs.size(); ++q)
            for (uint32_t i = 0; i < nhits[q]; ++i) {
                const mk_hit &h = hits[q * nres + i];
                const string &file_name = file_names[h.genome];
                vector<Pending> &v = batch[file_name];
                v.push_back(Pending{*seqs[q], heads[q], h.jaccard, h.intersection, h.genome});
                if (v.size() >= 100) { ground_truth(file_name, v); v.clear(); }
            }
        // the genome file of the NEXT entry is read and split while the device works on this one
        vector<const std::pair<const string, vector<Pending>> *> todo;
        for (auto itr = batch.begin(); itr != batch.end(); ++itr)
            if (!itr->second.empty()) todo.push_back(&*itr);
        std::future<GenomeContigs> ahead;
        // (a file whose set is still resident from a flush above is not read again)
        auto parse_unless_resident = [this](const string &f, bool res) { return res ? GenomeContigs{} : parse_contigs(f); };
        if (!todo.empty())
            ahead = std::async(std::launch::async, parse_unless_resident, todo[0]->first, is_resident(todo[0]->first, todo[0]->second));
        for (size_t i = 0; i < todo.size(); ++i) {
            GenomeContigs gc = ahead.get();
            if (i + 1 < todo.size())
                ahead = std::async(std::launch::async, parse_unless_resident, todo[i + 1]->first, false);
            ground_truth(todo[i]->first, todo[i]->second, gc);
        }
        out << flush;
    }

    // ---- Miekki.cpp:723-759
    void query_file_exact(const string &path)
    {
        if (!mkhost::file_exists(path)) { cout << "File problem" << endl; return; }
        if (!need_names()) return;
        vector<string> heads, seqs, kh;
        read_records(path, heads, seqs);
        vector<const string *> kept;
        for (size_t i = 0; i < seqs.size(); ++i)
            if (seqs[i].size() >= k && nucleotide_start(seqs[i])) { kept.push_back(&seqs[i]); kh.push_back(heads[i]); }
        exact_collect(kh, kept, 5, 10);
    }

    // ---- Miekki.cpp:616-645, 763-788
    void query_file_of_file_exact(const string &list)
    {
        if (!mkhost::file_exists(list)) { cout << "Missed file of file: " << list << endl; return; }
        if (!need_names()) return;
        string text;
        mkhost::read_text(list, text);
        vector<string> heads, refs;
        for (const string &fn : split_lines(text)) {
            if (fn.size() <= 3) continue;
            if (!mkhost::file_exists(fn)) {
                cout << "File problem" << endl;
            } else {
                string ftext;
                mkhost::read_text(fn, ftext);
                vector<string> lines = split_lines(ftext);
                string ref;
                for (size_t i = 1; i < lines.size(); ++i)
                    if (lines[i].size() >= k && nucleotide_start(lines[i])) ref += lines[i];   // 771-775
                heads.push_back(lines.empty() ? string() : lines[0]);
                refs.push_back(std::move(ref));
            }
            cout << "-" << flush_stream();
        }
        vector<const string *> ptrs;
        for (auto &r : refs) ptrs.push_back(&r);
        exact_collect(heads, ptrs, 5, 5);
    }
};

// the list of -K: one decimal genome id per line, blank lines ignored; false + why for anything else
bool read_keep_list(const string &path, vector<uint32_t> &ids, string &why)
{
    if (!mkhost::file_exists(path)) { why = "-K: cannot read " + path; return false; }
    string text;
    mkhost::read_text(path, text);
    std::unordered_set<uint32_t> seen;
    size_t line_no = 0;
    for (string line : split_lines(text)) {
        ++line_no;
        while (!line.empty() && isspace((unsigned char)line.back())) line.pop_back();
        size_t b = 0;
        while (b < line.size() && isspace((unsigned char)line[b])) ++b;
        line.erase(0, b);
        if (line.empty()) continue;
        const bool digits = line.size() <= 10 && line.find_first_not_of("0123456789") == string::npos;
        const unsigned long long v = digits ? strtoull(line.c_str(), nullptr, 10) : 0;
        if (!digits || v > 0xffffffffull) { why = "-K: line " + to_string(line_no) + " of " + path + " is not a genome id: " + line; return false; }
        if (!seen.insert((uint32_t)v).second) { why = "-K: genome id " + to_string(v) + " is listed twice in " + path; return false; }
        ids.push_back((uint32_t)v);
    }
    if (ids.empty()) { why = "-K: " + path + " lists no genome ids"; return false; }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 2) { help(); return 0; }
    // (the HIP runtime folds its streams onto four hardware queues unless told otherwise; the ingest has a dozen streams with
    // work at a time -- a batch's own, the upload streams, the build's -- and a copy that shares a queue with a long kernel of
    // another stream waits behind it: eight queues, unless the user has said something)
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    string index_file, list_file, query_lines, query_list, output_file("out.txt"), index_dump, keep_file, families_file, reps_file, clusters_file, profile_file, cover_file, winners_file, depth_file, gather_file, clades_file, clade_profile_file, panel_list, panel_file, taxonomy_file, lca_report_file, lca_reads_file, mates_file;
    long margin = 100, min_qual = -1;
    bool margin_given = false, qual_given = false;
    vector<string> join_files;                                   // -M, in the order given
    uint64_t H = 17, core_number = 8, kmer_size = 31, bloom_size = 33, fingerprint_size = 3;   // main.cpp:131
    double threshold = 200;
    bool exact_mode = false, threads_given = false, nres_given = false, index_queries = false;
    long nres = 10, min_new = 10;
    bool min_new_given = false;
    int c;
    while ((c = getopt(argc, argv, "i:l:a:h:t:f:k:s:b:o:ed:A:n:XK:F:R:r:M:P:C:W:D:G:g:L:p:S:c:T:y:Y:m:2:q:")) != -1) {
        switch (c) {
        case 'i': index_file = optarg; break;
        case 'l': list_file = optarg; break;
        case 'a': query_lines = optarg; break;
        case 'A': query_list = optarg; break;
        case 'o': output_file = optarg; break;
        case 'h': H = stoi(optarg); break;
        case 't': core_number = stoi(optarg); threads_given = true; break;
        case 'k': kmer_size = stoi(optarg); break;
        case 's': threshold = stof(optarg); break;
        case 'f': fingerprint_size = stoi(optarg); break;
        case 'b': bloom_size = stoi(optarg); break;
        case 'e': exact_mode = true; break;
        case 'd': index_dump = optarg; break;
        case 'n': nres = atol(optarg); nres_given = true; break;
        case 'X': index_queries = true; break;
        case 'K': keep_file = optarg; break;
        case 'F': families_file = optarg; break;
        case 'R': reps_file = optarg; break;
        case 'r': clusters_file = optarg; break;
        case 'M': join_files.push_back(optarg); break;
        case 'P': profile_file = optarg; break;
        case 'C': cover_file = optarg; break;
        case 'W': winners_file = optarg; break;
        case 'D': depth_file = optarg; break;
        case 'G': gather_file = optarg; break;
        case 'g': min_new = atol(optarg); min_new_given = true; break;
        case 'L': clades_file = optarg; break;
        case 'p': clade_profile_file = optarg; break;
        case 'S': panel_list = optarg; break;
        case 'c': panel_file = optarg; break;
        case 'T': taxonomy_file = optarg; break;
        case 'y': lca_report_file = optarg; break;
        case 'Y': lca_reads_file = optarg; break;
        case '2': mates_file = optarg; break;
        case 'q': { char *rest = nullptr; min_qual = strtol(optarg, &rest, 10); if (rest == optarg || *rest) min_qual = -1; qual_given = true; break; }
        case 'm': { char *rest = nullptr; margin = strtol(optarg, &rest, 10); if (rest == optarg || *rest) margin = -1; margin_given = true; break; }
        }
    }
    // -M: everything that can be refused is refused here, before a device is touched or a file is written
    if (!join_files.empty() && index_file.empty()) {
        cout << (list_file.empty() ? "-M joins index files to the index that -i loads: it needs -i"
                                   : "-M is not supported with -l: the joined genomes would have no file names (dump the build with -d, then -i ... -M ...)") << endl;
        return 1;
    }
    // -2: the mates of -a's records -- a pair is one query of the approximate mode and of every sink over -a's reads
    if (!mates_file.empty()) {
        if (query_lines.empty()) { cout << "-2 names the mates of the reads of a query file: it needs -a" << endl; return 1; }
        if (exact_mode || !query_list.empty() || index_queries || !panel_list.empty()) { cout << "-2 pairs the reads of -a for the approximate mode: it takes no -e, -A, -X or -S" << endl; return 1; }
        if (!mkhost::file_exists(mates_file)) { cout << "-2: cannot read " << mates_file << endl; return 1; }
    }
    // the sinks over the reads of -a likewise (-G's -g below): flag by flag, in this order
    struct SinkFlag { char letter; const string *path; const char *what, *how, *not_hits, *why_one; };
    const SinkFlag sinks[] = {
        {'P', &profile_file, "profiles the reads of a query file", "sums the approximate mode's answers over the reads of -a",
         "counts every genome above the thresholds and the best one per read", "a read's best genome is chosen among all of them"},
        {'p', &clade_profile_file, "profiles the reads of a query file by clade", "sums the approximate mode's answers over the reads of -a",
         "counts every clade above the thresholds and the best one per read", "a read's best genome is chosen among all of them"},
        {'y', &lca_report_file, "places the reads of a query file in a taxonomy", "places the approximate mode's answers for the reads of -a",
         "counts reads per node of the taxonomy, not hits per read", "a read's best genome is chosen among all of them"},
        {'C', &cover_file, "screens the reads of a query file", "counts the indexed fingerprints the reads of -a hold",
         "counts covered fingerprints per genome, not hits per read", "the table of seen cells lives on one device"},
        {'W', &winners_file, "screens the reads of a query file", "credits the cells the reads of -a hold to the indexed genomes",
         "counts the cells each genome wins, not hits per read", "the table of seen cells lives on one device"},
        {'D', &depth_file, "measures the depth of the reads of a query file", "counts the reads of -a that hold each indexed fingerprint",
         "reports a median and a sum per genome, not hits per read", "the table of counters lives on one device"},
        {'G', &gather_file, "gathers the genomes that explain the reads of a query file", "picks genomes by the cells the reads of -a hold",
         "reports every pick that explains at least -g new cells, not hits per read", "the table of seen cells lives on one device"},
    };
    for (const SinkFlag &f : sinks) {
        if (f.path->empty()) continue;
        if (query_lines.empty()) { cout << "-" << f.letter << " " << f.what << ": it needs -a" << endl; return 1; }
        if (exact_mode || !query_list.empty() || index_queries) { cout << "-" << f.letter << " " << f.how << ": it takes no -e, -A or -X" << endl; return 1; }
        if (nres_given) { cout << "-" << f.letter << " " << f.not_hits << ": it takes no -n" << endl; return 1; }
    }
    // -S / -c: the samples are the list's files, not -a's reads
    vector<string> panel_samples;
    if (panel_list.empty() != panel_file.empty()) {
        cout << (panel_file.empty() ? "-S screens the samples of a list: it needs -c, the file of their counts" : "-c receives the counts of the samples that -S lists: it needs -S") << endl;
        return 1;
    }
    if (!panel_list.empty()) {
        if (!query_lines.empty() || !query_list.empty() || exact_mode || index_queries) { cout << "-S takes its reads from the files of its list: it takes no -a, -A, -e or -X" << endl; return 1; }
        if (nres_given) { cout << "-S counts covered fingerprints per sample and genome, not hits per read: it takes no -n" << endl; return 1; }
        if (!mkhost::file_exists(panel_list)) { cout << "-S: cannot read " << panel_list << endl; return 1; }
        string text;
        mkhost::read_text(panel_list, text);
        mkhost::panel_list_files(text, panel_samples);
        if (panel_samples.empty()) { cout << "-S: " << panel_list << " names no file" << endl; return 1; }
        for (size_t i = 0; i < panel_samples.size(); ++i)
            if (!mkhost::file_exists(panel_samples[i])) { cout << "-S: cannot read sample " << i << " of " << panel_list << ": " << panel_samples[i] << endl; return 1; }
    }
    if (clade_profile_file.empty() != clades_file.empty()) {
        cout << (clades_file.empty() ? "-p profiles the reads by the clades of a file: it needs -L" : "-L names the clades that -p profiles the reads by: it needs -p") << endl;
        return 1;
    }
    if (lca_report_file.empty() != taxonomy_file.empty()) {
        cout << (taxonomy_file.empty() ? "-y reports the reads by the nodes of a taxonomy: it needs -T" : "-T names the taxonomy that -y reports the reads by: it needs -y") << endl;
        return 1;
    }
    if (!lca_reads_file.empty() && taxonomy_file.empty()) { cout << "-Y receives every read's node of a taxonomy: it needs -T" << endl; return 1; }
    if (margin_given && taxonomy_file.empty()) { cout << "-m is the margin of the placement in a taxonomy: it needs -T" << endl; return 1; }
    if (margin_given && (margin < 0 || margin > 100)) { cout << "-m takes a percentage, 0 .. 100" << endl; return 1; }
    if (min_new_given && gather_file.empty()) { cout << "-g is the least a pick of -G has to explain: it needs -G" << endl; return 1; }
    if (min_new_given && (min_new < 1 || min_new > 0xffffffffl)) { cout << "-g takes a number of cells from 1 on: with 0 the picks of -G would not end" << endl; return 1; }
    if (nres_given && (nres < 0 || nres >= (long)MK_LIST_CANDIDATES)) { cout << "-n takes a number of genomes per query, or 0 for all of them" << endl; return 1; }
    if (nres_given && exact_mode) { cout << "-n applies to the approximate mode only: -e reports the reference's hits" << endl; return 1; }
    if (index_queries && (exact_mode || !query_lines.empty() || !query_list.empty())) {
        cout << "-X queries the indexed genomes themselves: it takes no query file (-a, -A) and has no exact mode (-e)" << endl;
        return 1;
    }
    const vector<int> devices = mkhost::device_list();          // every visible GPU, or MIEKKI_DEVICES
    // one process per GPU?  (a launcher's environment: torch.distributed.run --no-python sets RANK / WORLD_SIZE / LOCAL_RANK)
    auto env_int = [](const char *a, const char *b, int dflt) { const char *e = getenv(a); if (!e) e = getenv(b); return e ? atoi(e) : dflt; };
    const int rank_world = env_int("MIEKKI_WORLD", "WORLD_SIZE", 1), rank_id = env_int("MIEKKI_RANK", "RANK", 0);
    const int rank_local = env_int("MIEKKI_LOCAL_RANK", "LOCAL_RANK", rank_id);
    const bool rank_mode = rank_world > 1 || getenv("MIEKKI_WORLD") != nullptr;
    if (rank_mode && (rank_id < 0 || rank_id >= rank_world)) { cout << "rank " << rank_id << " of " << rank_world << "?" << endl; return 1; }
    if (rank_mode && rank_id != 0) cout.setstate(std::ios_base::badbit);      // rank 0 speaks for all
    if (rank_mode && nres != 10) { cout << "-n other than 10 is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    if (rank_mode && index_queries) { cout << "-X is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    if (rank_mode && !keep_file.empty()) { cout << "-K is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    if (rank_mode && !families_file.empty()) { cout << "-F is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    const bool want_reps = !reps_file.empty() || !clusters_file.empty();
    if (rank_mode && want_reps) { cout << "-R / -r are not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    if (want_reps && devices.size() > 1) { cout << "-R / -r are not supported with several GPUs in the process: the rule goes through all ids in order (MIEKKI_DEVICES names one)" << endl; return 1; }
    // -q: the base-quality cut of the reads of -a (and -2) or of -S's samples -- FASTQ files, one GPU
    if (qual_given) {
        if (query_lines.empty() && panel_list.empty()) { cout << "-q cuts the reads of a query file at their bad bases: it needs -a or -S" << endl; return 1; }
        if (exact_mode || !query_list.empty() || index_queries) { cout << "-q cuts reads for the approximate mode: it takes no -e, -A or -X" << endl; return 1; }
        if (min_qual < 0 || min_qual > 93) { cout << "-q takes a phred quality, 0 .. 93" << endl; return 1; }
        vector<string> files;
        if (!query_lines.empty()) files.push_back(query_lines);
        if (!mates_file.empty()) files.push_back(mates_file);
        files.insert(files.end(), panel_samples.begin(), panel_samples.end());
        for (const string &f : files)
            if (mkhost::file_exists(f) && !mkhost::file_is_fastq(f)) { cout << "-q needs base qualities: " << f << " is not a FASTQ file (a first byte '@', a third line that starts with '+')" << endl; return 1; }
        if (rank_mode) { cout << "-q is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
        if (devices.size() > 1) { cout << "-q is not supported with several GPUs in the process: a set with qualities lives on one device (MIEKKI_DEVICES names one)" << endl; return 1; }
    }
    if (!mates_file.empty() && rank_mode) { cout << "-2 is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    if (!mates_file.empty() && devices.size() > 1) { cout << "-2 is not supported with several GPUs in the process: a set of pairs lives on one device (MIEKKI_DEVICES names one)" << endl; return 1; }
    for (const SinkFlag &f : sinks) {
        if (f.path->empty()) continue;
        if (rank_mode) { cout << "-" << f.letter << " is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
        if (devices.size() > 1) { cout << "-" << f.letter << " is not supported with several GPUs in the process: " << f.why_one << " (MIEKKI_DEVICES names one)" << endl; return 1; }
    }
    if (!panel_list.empty() && rank_mode) { cout << "-S is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    if (!panel_list.empty() && devices.size() > 1) { cout << "-S is not supported with several GPUs in the process: the table of the samples' cells lives on one device (MIEKKI_DEVICES names one)" << endl; return 1; }
    if (rank_mode && !join_files.empty()) { cout << "-M is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)" << endl; return 1; }
    if (!join_files.empty() && devices.size() > 1) { cout << "-M is not supported with several GPUs in the process: the two indexes are joined on one device (MIEKKI_DEVICES names one)" << endl; return 1; }
    vector<uint32_t> keep_ids;
    if (!keep_file.empty()) {
        string why;
        if (!read_keep_list(keep_file, keep_ids, why)) { cout << why << endl; return 1; }
    }
    mkhost::CladeList clade_list;
    if (!clades_file.empty()) {
        string text, why;
        if (!mkhost::file_exists(clades_file)) { cout << "-L: cannot read " << clades_file << endl; return 1; }
        mkhost::read_text(clades_file, text);
        if (!mkhost::parse_clades(text, clades_file, clade_list, why)) { cout << why << endl; return 1; }
    }
    mkhost::Taxonomy taxonomy;
    if (!taxonomy_file.empty()) {
        string text, why;
        if (!mkhost::file_exists(taxonomy_file)) { cout << "-T: cannot read " << taxonomy_file << endl; return 1; }
        mkhost::read_text(taxonomy_file, text);
        if (!mkhost::parse_taxonomy(text, taxonomy_file, taxonomy, why)) { cout << why << endl; return 1; }
    }
    const unsigned reader_threads = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(core_number, 64));
    const uint32_t bit_per_min = (uint32_t)(5 + fingerprint_size);                              // main.cpp:184
    cout << "Using " << bit_per_min << " bits per minimizer, " << int_to_string(1ull << H) << " minimizers so "
         << int_to_string((uint32_t)(bit_per_min * (1u << H))) << " bits per sequences" << endl;
    auto start = chrono::system_clock::now();
    Driver drv;
    drv.threads = reader_threads;
    drv.threads_given = threads_given;
    drv.nres = nres == 0 ? MK_ALL_RESULTS : (uint32_t)nres;
    drv.mates = mates_file;
    drv.min_qual = qual_given ? (int)min_qual : -1;
    if (rank_mode) {
        drv.rank_id = rank_id; drv.rank_world = rank_world; drv.rank_local = rank_local; drv.forced_rank_mode = true;
        drv.meet = mkhost::rendezvous_from_env();
        setenv("MIEKKI_COMM_BANNER_TO_STDERR", "1", 1);              // (stdout is compared with the reference's: mk_comm_create)
    }
    if (!index_file.empty()) {
        if (!mkhost::file_exists(index_file)) {
            cout << "File problem" << endl;
            return 1;
        }
        string err;
        vector<mk_ctx *> ctxs;
        // -M: the headers of all files first -- a file that is missing or was built with other parameters ends the run before
        // anything is loaded or joined -- and their genomes counted, so that the matrix is laid out once
        uint64_t join_genomes = 0;
        if (!join_files.empty()) {
            mk_params p0, p1;
            uint32_t g0 = 0, g1 = 0;
            if (!mkhost::read_index_header(index_file, p0, g0, err)) { cout << "Index load failed: " << err << endl; return 1; }
            for (const string &jf : join_files) {
                if (!mkhost::file_exists(jf)) { cout << "-M: cannot read " << jf << endl; return 1; }
                if (!mkhost::read_index_header(jf, p1, g1, err)) { cout << "-M: " << err << endl; return 1; }
                const char *differs = p1.k != p0.k ? "-k" : p1.h != p0.h ? "-h" : p1.fp_bits != p0.fp_bits ? "the fingerprint width (-f)"
                                    : p1.bloom_log2 != p0.bloom_log2 ? "-b" : nullptr;
                if (differs) { cout << "-M: " << jf << " and " << index_file << " were built with different parameters: " << differs << " differs" << endl; return 1; }
                join_genomes += g1;
            }
            if (g0 + join_genomes > 0xffffff00ull) { cout << "-M: " << g0 + join_genomes << " genomes are more than an index holds" << endl; return 1; }
        }
        if (rank_mode) {
            // one process per GPU: every rank reads the file and keeps the columns of its run of genomes (main.cpp:189-194,
            // Miekki.cpp:687-719 per rank).  A rank that cannot load still joins the communicator -- on a context of its
            // own making -- so that all ranks hear of it and leave together.
            const int device = rank_local < (int)devices.size() ? devices[rank_local] : rank_local;
            const bool loaded = mkhost::load_index(index_file, {device}, ctxs, err, reader_threads, rank_id, rank_world) == 0;
            if (!loaded) {
                mk_params p{31, 10, 8, 0, 0, device, 0, 0};
                mk_ctx *ctx = nullptr;
                if (mk_create(&p, &ctx) != MK_OK) die("cannot create a context");
                ctxs.assign(1, ctx);
            }
            drv.group.adopt(ctxs);
            drv.group.set_comm(drv.make_comm(ctxs[0]));
            drv.agree(loaded ? string() : (err.empty() ? string("unknown error") : err), "Index load failed: ");
        } else {
            if (mkhost::load_index(index_file, devices, ctxs, err, reader_threads, -1, 0, (uint32_t)join_genomes) != 0) { cout << "Index load failed: " << err << endl; return 1; }
            drv.group.adopt(ctxs);
        }
        drv.finish_index(false);                            // the file holds the global Bloom filter already
        mk_params p;
        mk_get_params(drv.ctx0(), &p);
        drv.k = p.k; drv.threshold = p.threshold;          // -k -h -f -b -s come from the file (main.cpp:189-194)
        for (const string &jf : join_files) drv.join_index(jf, devices[0]);
        if (!join_files.empty()) drv.compress_cold();       // (a join unpacks cold rows: INDEX->compress_index(1) once, after the last)
        if (!keep_ids.empty()) drv.keep_genomes(keep_ids);  // (a refused list leaves no output file behind)
        if (!rank_mode || rank_id == 0) drv.out.open(output_file.c_str());
        cout << "I output results in " << output_file << endl;
        cout << "Load sucessful" << endl;
    } else if (!list_file.empty()) {
        if ((!rank_mode || rank_id == 0) && keep_ids.empty()) drv.out.open(output_file.c_str());
        cout << "I output results in " << output_file << endl;
        drv.k = (uint32_t)kmer_size; drv.threshold = (uint32_t)threshold;
        drv.index_file_of_file(list_file, devices, [&](int device) {
            mk_params p{(uint32_t)kmer_size, (uint32_t)H, bit_per_min, (uint32_t)bloom_size, (uint32_t)threshold, device, 0, 0};
            mk_ctx *ctx = nullptr;
            const int st = mk_create(&p, &ctx);
            if (st == MK_ERR_UNSUPPORTED) { cout << "not implemented" << endl; exit(0); }          // Miekki.cpp:235-237
            if (st != MK_OK) die("cannot create the index");
            return ctx;
        });
        if (!keep_ids.empty()) {
            drv.keep_genomes(keep_ids);
            drv.compress_cold();                            // (the selection unpacks cold rows: INDEX->compress_index(1) once more)
            drv.out.open(output_file.c_str());
        }
    } else {
        cout << "What am I supposed to index ? use either -i or -l options please" << endl;
        help();
        return 0;
    }
    if (!families_file.empty()) drv.write_families(families_file);
    if (want_reps) drv.write_representatives(reps_file, clusters_file);
    if (!index_dump.empty()) {
        cout << "I write this index on the disk for later" << endl;
        string err;
        const int rc = rank_mode ? mkhost::dump_index_ranked(drv.ctx0(), drv.group.comm(), index_dump, err, reader_threads)
                                 : mkhost::dump_index(drv.group.contexts(), index_dump, err, reader_threads);
        if (rc != 0) { cout << "Index dump failed: " << err << endl; return 1; }
    }
    auto end_index = chrono::system_clock::now();
    cout << "elapsed time: " << chrono::duration<double>(end_index - start).count() << "s\n";
    if (!query_lines.empty()) {
        if (exact_mode) {
            cout << "running in exact mode, actual intersection will be computed on hits found by the index" << endl;
            drv.query_file_exact(query_lines);
        } else {
            cout << "running in approx mode, intersection is estimated by the index" << endl;
            if (!profile_file.empty() || !cover_file.empty() || !winners_file.empty() || !depth_file.empty() || !gather_file.empty() || !clade_profile_file.empty() ||
                !lca_report_file.empty()) {
                Driver::ProfileJob job;
                job.reads = query_lines;
                job.tally_path = profile_file; job.clade_path = clade_profile_file; job.clades = &clade_list;
                job.cover_path = cover_file; job.winners_path = winners_file; job.depth_path = depth_file;
                job.gather_path = gather_file; job.min_new = (uint32_t)min_new;
                job.tax_name = taxonomy_file; job.tax = &taxonomy; job.lca_path = lca_report_file; job.nodes_path = lca_reads_file; job.margin = (uint32_t)margin;
                drv.profile_file(job);
            }
            else drv.query_file(query_lines);
        }
    } else if (index_queries) {
        cout << "running in approx mode, intersection is estimated by the index" << endl;
        drv.query_index();
    } else if (!panel_list.empty()) {
        cout << "running in approx mode, intersection is estimated by the index" << endl;
        drv.panel_files(panel_samples, panel_file);
    } else if (!query_list.empty()) {
        if (exact_mode) {
            cout << "running in exact mode, actual intersection will be computed on hits found by the index" << endl;
            drv.query_file_of_file_exact(query_list);
        } else {
            cout << "running in approx mode, intersection is estimated by the index" << endl;
            drv.query_file_of_file(query_list);
        }
    } else {
        cout << "No query file, No queries" << endl;
    }
    auto end_query = chrono::system_clock::now();
    cout << "elapsed time: " << chrono::duration<double>(end_query - end_index).count() << "s\n";
    if (getenv("MIEKKI_VERBOSE") && (drv.group.shards() > 1 || drv.group.ranked()))
        cout << "[exchange] " << (drv.group.ranked() ? (size_t)drv.group.world() : drv.group.shards()) << " shards: " << drv.group.gather_bytes() << " bytes gathered, "
             << drv.group.rerun_queries() << " queries rerun with wide rows, " << drv.group.replayed_queries()
             << " answered from dense score rows" << endl;
    cout << "The end" << endl;
    drv.out.close();
    // One process, its work done and written: leave.  Taking the contexts apart first -- dozens of page-locked pieces, the device's
    // blocks, the streams, one runtime call each -- is 60-80 ms of a run that may be 300 (profiles/r6_cli_startup.txt), for memory
    // the driver takes back anyway when the process ends.  Ranks leave in order: their communicator is shared.
    if (!rank_mode) {
        for (mk_ctx *ctx : drv.group.contexts()) (void)mk_sync(ctx);   // (nothing of the library's is under way, on the device or on a thread)
        cout.flush();
        exit(0);                                             // (not _exit: a profiler's exit handlers write its files)
    }
    return 0;                                                // ~DeviceGroup releases the contexts
}
