// Internal declarations shared by the translation units of libmiekki_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/miekki_hip.h"
#include "mk_device.hpp"

namespace mk {

void set_error(const char *fmt, ...);
#define MK_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            mk::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,    \
                          __LINE__);                                                          \
            return e_ == hipErrorOutOfMemory ? MK_ERR_NOMEM : MK_ERR_DEVICE;                  \
        }                                                                                     \
    } while (0)
#define MK_TRY(expr)                                                                          \
    do {                                                                                      \
        int s_ = (expr);                                                                      \
        if (s_ != MK_OK) return s_;                                                           \
    } while (0)

constexpr uint32_t kShortMax = 4096;     // k-mers a query may have for the in-LDS sketch
}  // namespace mk
// ONE definition of "more k-mers than the short path takes" (len - k of them are sketched: Miekki.cpp:162 skips the last), used
// by a query set's own classes and by the callers that split a mixed set
struct mk_ctx;
namespace mk {
inline bool beyond_short_len(uint32_t k, uint64_t len) { return len > (uint64_t)k + kShortMax; }
// k-mers of a read pair: those of each mate alone (the last one of a sequence is skipped, Miekki.cpp:162)
inline uint64_t pair_kmers(uint32_t k, uint64_t len1, uint64_t len2) { return (len1 > k ? len1 - k : 0) + (len2 > k ? len2 - k : 0); }
constexpr uint32_t kBuildBatch = 64;     // most genomes sketched per build batch
constexpr uint32_t kTileBytes = 1024;    // bytes of one matrix row a wave scans (64 lanes x 16 B)
constexpr uint64_t kEmptyKey = ~0ULL;
constexpr int kPosBits = 40;                      // a minimum key in a table: fingerprint << 40 | position
constexpr int kCopyStreams = 2;                   // copy streams of a packed append (see mk_ctx::copy_extra; three: 30.9k sketches/s, four: 37.8k, two: 39.0k)
constexpr uint32_t kBloomRegionLog2 = 12;          // cells per region of the Bloom sweep (bloom_sweep_kernel): one pass of a workgroup

// packed query-sketch entry: partition in the low word, fingerprint in the high word
__host__ __device__ inline uint64_t make_entry(uint32_t p, uint32_t fp) { return (uint64_t)p | ((uint64_t)fp << 32); }

struct Timer {
    hipEvent_t a, b;
    int kind;            // 0 sketch, 1 scan, 2 filter, 3 build sketch, 4 build finalize
};

// gz_pool.hip: the inflater keeps its batches' device blocks for the next batches (tens of gigabytes after an ingest of gzip'd
// genomes); whoever finds device memory short gives the idle ones back -- every context's -- and tries again
uint64_t gz_release_idle_blocks();
template <typename T>
inline int dev_alloc(T **p, uint64_t count)
{
    *p = nullptr;
    if (!count) return MK_OK;
    if (hipMalloc((void **)p, count * sizeof(T)) == hipSuccess) return MK_OK;
    (void)hipGetLastError();
    *p = nullptr;
    if (gz_release_idle_blocks() == 0) { set_error("HIP error: out of memory (%llu bytes)", (unsigned long long)(count * sizeof(T))); return MK_ERR_DEVICE; }
    MK_HIP(hipMalloc((void **)p, count * sizeof(T)));
    return MK_OK;
}
template <typename T>
inline void dev_free(T *&p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}
// a device allocation that lasts as long as a scope: DevGuard<T> guard(d_p) frees d_p (null: nothing) on the way out
struct DevFree { void operator()(void *p) const { (void)hipFree(p); } };
template <typename T> using DevGuard = std::unique_ptr<T, DevFree>;
// The one way a device array grows: room for `need` elements -- when there is less, the array is replaced (its contents are
// not kept) by one of need + slack.  A failed allocation leaves an empty array.  A caller whose array may still be read by
// queued work waits for that work first.  (For the arrays of a query set; a context's are DevArrays.)
template <typename T>
inline int dev_grow(T *&p, uint64_t &cap, uint64_t need, uint64_t slack = 0)
{
    if (need <= cap) return MK_OK;
    dev_free(p);
    cap = 0;
    MK_TRY(dev_alloc(&p, need + slack));
    cap = need + slack;
    return MK_OK;
}

// ---- what a context owns: move-only, released with their owner, read as the plain pointer / handle wherever one is wanted
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};
// A device array and the elements it has room for.  alloc replaces it (contents are not kept; a failed allocation leaves it
// empty) by one of count elements plus `pad` more that do not count as room: what kernels read or keep behind the array's
// end.  grow is dev_grow.
template <typename T>
struct DevArray : NoCopy {
    T *p = nullptr;
    uint64_t cap = 0;
    DevArray() = default;
    DevArray(DevArray &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevArray &operator=(DevArray &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevArray() { reset(); }
    operator T *() const { return p; }
    T *operator->() const { return p; }
    void reset() { dev_free(p); cap = 0; }
    int alloc(uint64_t count, uint64_t pad = 0)
    {
        reset();
        MK_TRY(dev_alloc(&p, count + pad));
        cap = count;
        return MK_OK;
    }
    int grow(uint64_t need, uint64_t slack = 0) { return need <= cap ? MK_OK : alloc(need + slack); }
};
// page-locked host memory from hipHostMalloc, likewise
template <typename T>
struct PinnedArray : NoCopy {
    T *p = nullptr;
    uint64_t cap = 0;
    PinnedArray() = default;
    PinnedArray(PinnedArray &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinnedArray &operator=(PinnedArray &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~PinnedArray() { reset(); }
    operator T *() const { return p; }
    T *operator->() const { return p; }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    int alloc(uint64_t count)
    {
        reset();
        MK_HIP(hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault));
        cap = count;
        return MK_OK;
    }
};
struct Stream : NoCopy {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    int create(unsigned flags = hipStreamDefault) { MK_HIP(hipStreamCreateWithFlags(&s, flags)); return MK_OK; }
};
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    int create(unsigned flags = hipEventDisableTiming) { if (!e) MK_HIP(hipEventCreateWithFlags(&e, flags)); return MK_OK; }   // (once; none of them is timed)
};

}  // namespace mk

#include "gz_pool.hpp"

// Where the rows of the fingerprint matrix live (SURVEY 8f row N4 -- what compress_index /
// decompress_index were for in the reference, Miekki.cpp:863-877: a collection larger than fast
// memory).  Rows [0, P_hot) are in HBM; when the matrix exceeds its HBM budget the remaining COLD
// rows sit in page-locked host memory (device-visible).  Kernels address row p through mat_row;
// the slab schedule streams whole cold partition ranges through a staging buffer in HBM instead
// of reading them piecemeal over PCIe (api_query.hip: qset_scan_slab).
struct MatRef {
    uint8_t *hot;                  // row p < P_hot at hot + p * ld
    uint8_t *cold_m;               // row p >= P_hot at cold_m + p * ld (= cold rows' base - P_hot * ld); null when all rows are hot
    uint32_t P_hot;
};
__device__ __forceinline__ uint8_t *mat_row(const MatRef &m, uint32_t p, uint64_t ld)
{
    return (p < m.P_hot ? m.hot : m.cold_m) + (uint64_t)p * ld;
}

namespace mk {
// how the binned build lays a batch out in a side's slots (build.hip: build_setup)
struct BuildShape {
    uint32_t nbins, low_bits;      // low_bits = min(h, 12) partitions per bin (log2); nbins = P >> low_bits
    uint32_t lpr;                  // lanes of a reduce wave that share one run, 16 bytes of items each (a power of two)
    uint32_t nwg;                  // scatter workgroups per genome
    uint32_t tune;                 // 0 in the shipped library; timing experiments of a -DMK_TUNE_BUILD build: 1 no Bloom pass A, 2 no item reads
    uint32_t sum_words;            // 64-bit words of the Bloom summary the scatter kernel consults (one bit per 2048 cells); 0: none
    uint32_t bloom_on;             // the index has a Bloom filter (and pass A is not switched off): items get flagged
    uint32_t tables_only;          // query sketches: the reduce kernel leaves the minimum keys in `tables` and nothing else
};
// The long, mid-length and dense query sketches keep their per-query counters (kCountStride words apart) and per-workgroup
// partial sums in one block of the context: mk_ctx::d_sketch_scratch, this many 32-bit words (16 MiB)
constexpr uint32_t kSketchScratchWords = 1u << 22;
}  // namespace mk

// Everything a context holds on the device, in page-locked memory, as a stream or as an event is a member that releases
// itself (mk::DevArray, PinnedArray, Stream, Event); ~mk_ctx (api.hip) does the few things that are not.
struct mk_ctx {
    mk_params p{};
    uint32_t P = 0, W = 0, f = 0, empty = 0;
    mk::Stream stream;
    // fingerprint matrix, partition-major: row p at d_M + p * ld (bytes); 16-bit values native LE
    // (d_M, h_M, d_sketch_size and d_genome_size are plain pointers: ensure_capacity makes their successors beside them and
    // swaps all four at once; h_Z too, which cold.hip hands over the same way)
    uint8_t *d_M = nullptr;
    uint64_t ld = 0;
    uint8_t *h_M = nullptr;        // cold rows [P_hot, P) in page-locked host memory, same pitch (null: all rows in HBM)
    uint32_t P_hot = 0;            // rows kept in HBM (= P when the matrix fits its budget)
    uint64_t hbm_matrix_budget = 0;   // bytes of HBM the matrix may take (MIEKKI_HBM_MATRIX_MIB; 0 = whatever is free)
    // the cold rows PACKED (cold.hip: mk_index_compress): h_M is null then, h_Z holds them, row i of the cold rows at
    // h_Z + h_zoff[i]; d_zoff = the same offsets on the device; d_zstage = packed staging beside d_cold_stage's halves
    uint8_t *h_Z = nullptr;
    uint64_t z_bytes = 0;
    mk::DevArray<uint64_t> d_zoff;
    std::vector<uint64_t> h_zoff;
    mk::DevArray<uint8_t> d_zstage[2];
    mk::DevArray<uint8_t> d_cold_stage;   // HBM staging for cold partition ranges (slab schedule)
    uint64_t cold_stage_rows = 0;  // rows of ONE of its two halves
    mk::Event ev_cold[5];          // copy done [2], scan done [2], entry
    uint32_t capG = 0, G = 0;
    uint32_t *d_sketch_size = nullptr;
    uint64_t *d_genome_size = nullptr;
    mk::DevArray<float> d_ratio;   // genome_size / sketch_size (select.hip), capG entries, current as of ratio_gen
    uint64_t ratio_gen = 0;
    mk::DevArray<uint8_t> d_colstage;   // staging of mk_index_export_columns / _import_columns (kept between calls)
    mk::DevArray<uint8_t> d_huff;  // mk_index_import_columns_huffman: coded bytes, block list, code lengths, remainders (kept between calls)
    mk::DevArray<uint8_t> exact_buf[10];   // exact mode (K7) scratch, grown on demand
    bool exact_have_B = false;     // set B of the genome loaded last (mk_exact_load_genome) is resident
    uint64_t exact_nB = 0;         // its number of distinct k-mers
    uint32_t exact_log2B = 0;
    bool has_empty_sketch = false; // some genome has sketch_size 0 (see nan_candidates_possible in api_query.hip)
    bool next_single = false;      // the batch being queued comes from mk_index_insert_sequence
    // sizes of ALL genomes of a sharded index (mk_merge_set_sizes), for the compact merge on the
    // context that receives the gathered rows
    mk::DevArray<uint32_t> d_all_ss;
    mk::DevArray<uint64_t> d_all_gs;
    uint32_t all_n = 0, all_base = 0;
    uint64_t gen = 1;              // index generation: bumped whenever genomes or Bloom cells change
    uint64_t index_id = 0;         // which genome an id names: advanced by mk_index_select and mk_index_import_begin (sets made by
                                   // mk_qset_from_index remember it: mk_qset::index_id)
    std::vector<uint32_t> h_sketch_size;
    std::vector<uint64_t> h_genome_size;
    // Bloom filter: only the cells a 2k-bit k-mer can reach live on the device
    mk::DevArray<uint8_t> d_bloom;
    uint64_t bloom_dev_bytes = 0, bloom_bytes = 0;
    mk::DevArray<uint32_t> d_bloom_order;   // first-writer arbitration keys (build only), lazily allocated: one per reachable cell,
                                   // (genome in batch << h | partition) << 3 | bit of the first k-mer (in that order) that asked for the cell
    // build scratch (lazily allocated)
    uint32_t build_batch = 0;      // genomes per build batch (<= kBuildBatch, bounded by table memory)
    mk::DevArray<uint64_t> d_tables;   // build_batch x P min-keys
    mk::DevArray<uint32_t> d_sketch_scratch;   // kSketchScratchWords: the query sketches' counters and partial sums
    // batch sequences, concatenated.  Two buffers: while the kernels of one batch run out
    // of one, the next batch is copied into the other on copy_stream (mk_index_append)
    mk::DevArray<char> d_seq[2];   // (64 bytes behind each)
    int seq_cur = 1;               // buffer of the batch enqueued last
    // one bit per 8 Bloom cells: all eight are non-zero (so none of them can change any more).
    // 1 MiB for the 64 MiB of reachable cells at -b 33: L2-resident, and once the filter has
    // filled up it answers almost every probe of the build without touching the cells
    mk::DevArray<uint32_t> d_bloom_full;
    mk::DevArray<uint64_t> d_bloom_full2;   // coarse level: one bit per 2048 cells = all of them are taken (the build's scatter kernel asks it)
    bool bloom_full_stale = true;  // the cells were written behind the summary's back (import)
    mk::Stream copy_stream;
    mk::Event ev_copy;
    // further copy streams for batches that arrive as many separate buffers (mk_index_append_packed: one per sequence,
    // ~1 MB each): a DMA engine spends as long on starting such a copy as on moving it, several engines overlap that
    static constexpr int kCopyExtra = mk::kCopyStreams - 1;
    mk::Stream copy_extra[kCopyExtra];
    mk::Event ev_extra[kCopyExtra];
    // The batch whose kernels are enqueued but whose results (active counts, cardinality
    // sums) the host has not folded into the index yet.  Every entry point
    // other than the appends settles it first (settle_build in api.hip).
    struct BuildInFlight {
        bool on = false, binned = false;
        bool have_chars = false;   // the batch's characters are in d_seq[buf] (else only its packed form exists, in d_pk[buf])
        bool have_heads = false;   // d_heads[buf] holds the sequences' first 32 characters (packed input)
        bool single = false;       // mk_index_insert_sequence: the size estimate of Miekki.cpp:243-273 (active count in a double)
        uint32_t n = 0;
        uint32_t g0 = 0;           // its first column of the matrix (set when the back stage is queued)
        int buf = 0;
        uint64_t off[mk::kBuildBatch + 1] = {};
    } build, older, front;         // build: the batch whose back stage was queued last; older: the one before it, not folded
                                   // in yet (its back stage is running or done); front: front stage queued, back stage not
    uint32_t G_back = 0;           // genomes whose back stage has been queued: G + those of `older` and `build`
    // The batch in packed form (build.hip): d_pk[b] = [codes: d_pk[b].cap bytes][exception bits: half as many][256 bytes],
    // sequence g at byte offset pk_off[g] (16-byte aligned) of the codes and pk_off[g] / 2 of the exception bits.
    // Two of everything: the next batch is generated or copied into one while the kernels of the batch in flight
    // read the other.
    mk::DevArray<uint8_t> d_pk[2];
    uint8_t *pk_except(int b) const { return d_pk[b].p + d_pk[b].cap; }
    mk::DevArray<uint64_t> d_pk_off[2];   // kBuildBatch + 1 offsets
    mk::DevArray<char> d_heads[2]; // kBuildBatch x 32 characters
    // host images of the small per-batch arrays: they are copied asynchronously, and an append returns with its
    // batch still in flight, so they live here and not on a caller's stack
    // (page-locked: a copy from pageable memory makes the host wait until the stream has reached it -- for the
    // front stream that is the end of the batch's PCIe copy)
    struct HostImages {
        uint64_t pk_off[2][mk::kBuildBatch + 1];
        uint64_t off[2][mk::kBuildBatch + 1];
        uint32_t dirty[2][mk::kBuildBatch];
        char heads[2][mk::kBuildBatch * 32];
    };
    mk::PinnedArray<HostImages> h_img;
    // Per-batch counters of the build live in ONE device block (one memset before a batch, one copy
    // back after it).  BuildCounters is its layout, and that of the pinned read-back block.
    struct BuildCounters {
        uint32_t dirty[mk::kBuildBatch];   // some character is not A, C, G or T
        uint32_t act[mk::kBuildBatch];     // non-empty partitions
        uint64_t card[mk::kBuildBatch];    // sum of 2^(31-exp)
    };
    // The build runs as a two-stage pipeline over two SIDES (build.hip): the FRONT stage of a batch -- packing,
    // seed digits, scatter: instruction-bound -- is queued on front_stream while the BACK stage of the batch before
    // it -- reduce, matrix rows, Bloom passes: bound by memory latency -- still runs on `stream`; the two kinds of
    // kernels share the CUs.  Everything a front stage writes is per side, and whoever launches on a side names it.
    // The long-query sketches, which run only when no batch is in flight, use side 0.
    struct BuildSide {
        mk::DevArray<BuildCounters> d_counters;
        mk::PinnedArray<BuildCounters> h_back;   // pinned, so that the copy back does not block the host
        mk::DevArray<uint64_t> d_seq_off;        // kBuildBatch + 1
        mk::DevArray<uint32_t> d_seed_valid;     // kBuildBatch
        mk::Event ev_back;         // the batch's back stage (and its counters' copy back) is done
        mk::DevArray<uint8_t> d_slots;           // (1 KiB + 64 bytes behind them: build_setup)
        mk::Event ev_front;        // front stage done
        mk::BuildShape shape{};    // of the batch (build_setup)
        bool fits = false, key32 = false;
    } side[2];
    mk::Stream front_stream;
    // sizes of the batch just settled on their way to the device (pinned, one per buffer parity: the copy
    // is queued, not waited for)
    struct SizeUpload { uint32_t ss[mk::kBuildBatch]; uint64_t gs[mk::kBuildBatch]; };
    mk::PinnedArray<SizeUpload> h_sizes;
    int size_parity = 0;
    // query scratch
    mk::DevArray<uint32_t> d_scores;     // score matrix of the query chunk in flight
    mk::DevArray<uint8_t> d_partials;    // slab schedule: per-range mismatch counts of the chunk in flight
    mk::DevArray<uint32_t> d_flag;       // one word for device-side eligibility checks
    // mk_query's chunk: entrants per query, and the K6b output [queries][nresults]
    mk::DevArray<uint32_t> d_count;
    mk::DevArray<mk_hit> d_cand;
    mk::DevArray<mk_hit> d_hits;
    mk::DevArray<uint32_t> d_nhits;
    // scratch of the query lists (list.hip; mk_query_list / mk_qset_run_list), grown on demand: per-query counts and their
    // two scans, the compacted records, the heaps (key, ref) and the gathered hits of the queries in flight
    struct ListScratch {
        mk::DevArray<uint32_t> d_count;
        mk::DevArray<uint64_t> d_off;    // [2][queries of the chunk + 1]: record offsets, result offsets
        mk::DevArray<uint64_t> d_rec;
        mk::DevArray<double> d_key;
        mk::DevArray<uint32_t> d_ref;
        mk::DevArray<mk_hit> d_hits;
    } list;
    // scratch of the link pass (family.hip): the ids the queries of the set in flight stand for, the labels on their way out
    struct LinkScratch {
        mk::DevArray<uint32_t> d_qid;
        mk::DevArray<uint32_t> d_label;
    } link;
    // scratch of the representatives pass (rep.hip): the bitmap rows of the set in flight, rep[G] and the bitmap of the
    // final representatives
    struct RepScratch {
        mk::DevArray<uint32_t> d_rows;
        mk::DevArray<uint32_t> d_rep;
        mk::DevArray<uint32_t> d_is_rep;
    } rep;
    // small calls (mk_query with a handful of queries) are round trips, not kernels: one cached
    // device arena for the call's transient query set, one pinned block for its upload image and
    // one for its results, so that a call is one copy in, the kernels, one sync, one copy out
    mk::DevArray<uint8_t> d_qarena;
    bool qarena_busy = false;
    mk::PinnedArray<uint8_t> h_stage;
    mk::PinnedArray<uint8_t> h_res;
    mk::DevArray<uint64_t> d_long_table; // P keys, long-query path
    mk::DevArray<uint8_t> d_fpT;   // build: fingerprints of the batch, genome-major [build_batch][P] (fused build kernel)
    mk::DevArray<uint8_t> d_bloom_touched;   // build: per region of 2^kBloomRegionLog2 cells "a first-writer key was posted here" (allocated with d_bloom_order),
                                   // and behind those flags (bloom_regions(c) of them) "swept since the last summary": what bloom_summary_kernel redoes
    // stats
    mk_stats stats{};
    std::vector<mk::Timer> pending;
    std::vector<mk::Timer> free_timers;
    mk::GzPool gz;                 // what the gzip inflater keeps between batches (the last member: it goes first)
    ~mk_ctx();                     // api.hip: the matrix, the timers' events (mk_destroy has quiesced the device)
};

namespace mk {
struct DenseLut; struct mk_gz_stream; struct mk_gz_seg;
// the list of a (query block, partition range) for scan_block_kernel (scan_kernel.hpp): npackets 16-byte packets from packet `base` on,
// the zero packets that pad the list to whole steps (kBlockStepPackets) included
struct BlockInfo { uint64_t base; uint32_t npairs, npackets; };
// which kernel walks a set's partition ranges (scan.hip: launch_scan_slab).  Chosen once per preparation of a set, by
// qset_prepare_slab (api_query.hip)
enum class RangedScan : uint32_t {
    ByCount,    // small sets: ranges cut by entry count, no range table -- scan_slab_kernel
    PerWave,    // range table, one query per wave -- scan_slab_kernel
    Groups,     // range table, groups of kGroupQ queries per wave from their merged lists -- scan_group_kernel
    Blocks,     // range table, blocks of block_q queries per workgroup from their packets -- scan_block_kernel
};
}
struct mk_qset {
    uint32_t nq = 0;
    mk_ctx *owner = nullptr;
    bool arena_borrowed = false;   // d_arena is the context's cached arena (transient sets of mk_query)
    uint64_t head_bytes = 0;       // arena bytes [0, head_bytes) = sequences, offsets, entry offsets: the upload image
    uint64_t o_off = 0, o_ent_off = 0;   // byte offsets of d_off / d_ent_off in the arena (d_seq is at 0)
    uint8_t *d_arena = nullptr;    // the set's one device allocation; the arrays below point into it
    bool split_in_arena = false;   // d_split too (room for split_room ranges), else it is its own allocation
    uint32_t split_room = 0;
    char *d_seq = nullptr;
    uint64_t total_len = 0;
    uint64_t *d_off = nullptr;     // nq + 1 offsets into d_seq
    uint64_t *d_ent_off = nullptr; // nq + 1 offsets into d_entries (capacity max(len-k,0) each)
    uint64_t *d_entries = nullptr;
    uint32_t *d_nent = nullptr;    // active partitions per query
    std::vector<uint64_t> h_off, h_ent_off;
    std::vector<uint32_t> long_q;  // queries with more than kShortMax k-mers (sparse long path)
    // dense long path: queries with >= P/4 k-mers (whole genomes) keep their full 2^h
    // fingerprint vector, four queries interleaved per group: dense[group][p][4] (W bytes each)
    std::vector<uint32_t> dense_q; // set indices, group-major; 0xffffffff pads the last group
    uint8_t *d_dense = nullptr;
    uint32_t *d_dense_q = nullptr;
    mk::DenseLut *d_dense_lut = nullptr;   // one-byte fingerprints: the dense queries' field tables, [octet][P] (scan_kernel.hpp)
    uint32_t *d_scan_n = nullptr;  // entries the sparse scan walks: nent for sparse queries, 0 for dense ones
    uint32_t short_max_nk = 0;     // longest short query (k-mers)
    // A set of READ PAIRS (mk_qset_upload_pairs): query q is the two mates back to back in d_seq, d_cut[q] = mate 1's
    // length.  Only the short sketch knows (sketch.hip: query_sketch_pairs_kernel); null in every other set.
    uint32_t *d_cut = nullptr;
    // A set WITH BASE QUALITIES (mk_qset_upload_reads): d_qual holds the phred + 33 bytes in d_seq's layout, min_qual the
    // threshold below which a base cuts its read.  The short sketch's masked arm does the cutting; with d_cut the set is one of
    // pairs with qualities.  Null in every other set.
    uint8_t *d_qual = nullptr;
    uint32_t min_qual = 0;
    uint32_t *d_split = nullptr;   // [nq][S + 1] entry index of each partition-range boundary
    uint32_t S = 0;                // ranges of the slab schedule (0 = not prepared)
    uint32_t chunk = 0;            // ranges cut by count: entries per range
    bool slab_ok = false;          // every (query, range) fits the packed counters
    mk::RangedScan ranged = mk::RangedScan::PerWave;   // slab_ok: the kernel that walks the ranges
    uint64_t *d_glist = nullptr;   // the query groups' merged lists for scan_group_kernel (ent_off[nq] entries)
    // the query blocks' lists for scan_block_kernel (scan_kernel.hpp): packets, and where each (block, range) has its own
    uint4 *d_bpackets = nullptr;
    mk::BlockInfo *d_binfo = nullptr;
    uint64_t bpackets_cap = 0, binfo_cap = 0;
    uint32_t block_q = 0;          // queries per block of the lists in d_bpackets
    uint32_t block_sub_fast = 0;   // the order their work items are walked in (SlabArgs::block_sub_fast), set with block_q
    bool sketched = false;
    uint64_t gen = 0;              // index generation the sketch / range table were made against
    // A MIXED set (short queries next to long reads / contigs / whole genomes; query_file batches whatever the file holds,
    // Miekki.cpp:465-471) is a shell over two sets of its own -- the short queries, which keep the slab schedule, and the
    // others, which take the plain / dense kernels: part[i] runs as a set, part_q[i] = its queries' places in this set
    // (ascending), d_part_q[i] the same on the device, and the parts' rows are put in their places behind the parts' runs.
    mk_qset *part[2] = {nullptr, nullptr};
    std::vector<uint32_t> part_q[2];
    uint32_t *d_part_q[2] = {nullptr, nullptr};
    uint8_t *d_part_out = nullptr;  // a part's output rows before they go to their places
    uint64_t part_out_bytes = 0;
    // A set made from STORED COLUMNS (colq.hip; mk_qset_from_index / mk_qset_from_columns): every query dense, no sequences
    // (d_seq is null).  From the index: col_ids = the queries' columns (local genome ids), and the set's "sketch" step is
    // the gather of those columns, redone whenever the index changes.  From a caller's columns: d_dense and d_nent were
    // filled when the set was made and ARE the set's copy of them -- nothing is ever gathered again.
    bool columns = false, from_index = false;
    std::vector<uint32_t> col_ids;
    uint32_t *d_col_ids = nullptr;
    uint64_t index_id = 0;               // from_index: the context's index_id when the set was made -- another value: the ids name other genomes
    uint32_t *d_col_partial = nullptr;   // [nq][column_blocks] partial counts of non-empty partitions
};

namespace mk {

inline MatRef mat_ref(const mk_ctx *c)
{
    MatRef m;
    m.hot = c->d_M;
    m.P_hot = c->P_hot;
    m.cold_m = c->h_M ? c->h_M - (uint64_t)c->P_hot * c->ld : nullptr;
    return m;
}

// the tiles of a row that hold genomes; the kernels that walk a row tile by tile load whole tiles, which the pitch must cover
inline int row_tiles(const mk_ctx *c, uint32_t *ntiles)
{
    *ntiles = (uint32_t)(((uint64_t)c->G * c->W + kTileBytes - 1) / kTileBytes);
    if ((uint64_t)*ntiles * kTileBytes > c->ld) { set_error("the matrix rows do not cover whole tiles"); return MK_ERR_STATE; }
    return MK_OK;
}

// parameters every sketch kernel takes
struct SketchParams {
    uint32_t k, h, f, empty, bloom_log2, P;
    uint64_t kmask;
};
inline SketchParams make_sp(const mk_ctx *c)
{
    SketchParams s;
    s.k = c->p.k; s.h = c->p.h; s.f = c->f; s.empty = c->empty; s.bloom_log2 = c->p.bloom_log2;
    s.P = c->P;
    s.kmask = (c->p.k < 32) ? ((1ULL << (2 * c->p.k)) - 1) : ~0ULL;
    return s;
}

// timing helpers (api.hip)
int timer_begin(mk_ctx *c, int kind, Timer &t, hipStream_t stream = nullptr);
int timer_end(mk_ctx *c, Timer &t, hipStream_t stream = nullptr);
int drain_timers(mk_ctx *c);
struct ScopedTimer {
    mk_ctx *c; Timer t; bool on; hipStream_t stream;
    ScopedTimer(mk_ctx *ctx, int kind, hipStream_t st = nullptr) : c(ctx), on(false), stream(st) { on = timer_begin(c, kind, t, stream) == MK_OK; }
    ~ScopedTimer() { if (on) (void)timer_end(c, t, stream); }
};

// ---- api.hip, for its sister files (api_query.hip, api_sinks.hip, api_multi.hip)
// Every entry point starts here: bind the device and, unless the caller is an append that wants to overlap with it, fold
// the build batches still in flight into the index.
int use_device(const mk_ctx *c, bool settle = true);
int settle_build(mk_ctx *c);
// for_append = false: the long-query sketches borrow the tables, side 0 and their own scratch only
int ensure_build_scratch(mk_ctx *c, uint64_t seq_bytes, int buf = 0, bool for_append = true);

// ---- sketch.hip
int launch_genome_sketch(mk_ctx *c, const char *d_seq, const uint64_t *d_off, const uint64_t *h_off,
                         const uint32_t *d_valid, uint32_t n, uint64_t *d_tables);
// the character path's passes over a batch's tables: the sums go to side sd's counters, the offsets and seeds' validity are its own
int launch_finalize(mk_ctx *c, mk_ctx::BuildSide &sd, const uint64_t *d_tables, uint32_t n, uint32_t g0);
int launch_bloom_insert(mk_ctx *c, const mk_ctx::BuildSide &sd, uint64_t *d_tables, const char *d_seq, uint32_t n);
// Page-locked host memory for the ingest's buffers (api.hip): ordinary memory in transparent huge pages, registered with the
// runtime -- a 16 MiB piece is 8 pages to pin instead of 4,096, and the page faults are the calling thread's own, where sixteen
// reader threads asking hipHostMalloc for their first pieces stood in one queue for 70 ms (profiles/r6_cli_startup.txt).
// hipHostMalloc when that does not work.  pinned_free takes either kind.
void *pinned_alloc(uint64_t bytes);
void pinned_free(void *p);
int launch_bloom_summary(mk_ctx *c, bool after_sweep = false);   // after_sweep: only the regions the sweep has just changed, when the rest is current
uint64_t bloom_regions(const mk_ctx *c);                          // flags per array of d_bloom_touched
int launch_build_tail(mk_ctx *c, uint32_t n, uint32_t g0);     // matrix rows, Bloom pass B, summary (after a fused reduce kernel)
// ---- build.hip: the index build from packed sequences (2-bit codes + exception bits)
// (these four run on c->front_stream, on side b's arrays; launch_unpack on c->stream)
int launch_pack(mk_ctx *c, int b, const char *d_seq, const uint64_t *h_off, uint32_t n, uint8_t *d_codes, uint8_t *d_except,
                const uint64_t *d_code_off, hipStream_t st = nullptr);       // st: the front stream unless given
int launch_seed_fix(mk_ctx *c, int b, const char *d_seq, const char *d_heads, uint32_t n, uint8_t *d_codes, uint8_t *d_except,
                    const uint64_t *d_code_off, hipStream_t st = nullptr);
int launch_synth_packed(mk_ctx *c, uint64_t first_id, uint32_t n, uint64_t len, uint8_t *d_codes, const uint64_t *d_code_off,
                        uint32_t strains = 0, uint32_t rate_ppm = 0);      // strains != 0: related genomes (mk_device.hpp: strain_word)
int launch_unpack(mk_ctx *c, int b, const uint8_t *d_codes, const uint8_t *d_except, const uint64_t *d_code_off, const char *d_heads,
                  const uint64_t *h_off, uint32_t n, char *d_seq);
// front stage of a batch on c->front_stream: the scatter kernel into side `b` (*used = false: the shape does not suit
// the bins, nothing was launched); back stage on c->stream: reduce + fingerprints + sizes + Bloom pass A, matrix rows,
// Bloom pass B, summary
int launch_build_front(mk_ctx *c, int b, const uint8_t *d_codes, const uint8_t *d_except, const uint64_t *d_code_off,
                       const uint64_t *h_off, uint32_t n, bool *used, hipStream_t st = nullptr, bool for_queries = false);
// K1 of a run of long queries through the build's packed kernels (side 0, c->stream; no build is in flight when a query
// runs): d_tables[q][p] = fingerprint << kPosBits | position of partition p's minimum, kEmptyKey where there is none; the
// queries' packed form stays in c->d_pk[0] (offsets c->d_pk_off[0], "has exceptions" flags in side 0's counters) for the
// kernels that gate the winners.  *used = false: the shape does not fit the bins, nothing was written.
int launch_query_tables(mk_ctx *c, const char *d_seq, const uint64_t *d_off, const uint64_t *h_off, uint32_t n, uint64_t *d_tables,
                        bool *used);
uint64_t packed_offsets(const uint64_t *h_off, uint32_t n, uint64_t *pk_off);
int ensure_packed(mk_ctx *c, int buf, uint64_t code_bytes);
int launch_build_back(mk_ctx *c, int b, const uint8_t *d_codes, const uint8_t *d_except, const uint64_t *d_code_off, uint32_t n,
                      uint32_t g0);
int ensure_build_side(mk_ctx *c, int b);
int launch_bloom_merge(mk_ctx *c, uint64_t begin, uint64_t end, const uint8_t *d_later);
// api_query.hip: one pass of the hot path over a query set (mk_qset_run / mk_qset_run_compact; comm.hip hooks the chunks)
int qset_run(mk_ctx *c, mk_qset *qs, uint32_t nresults, uint32_t min_score, double min_inter, uint32_t cap, uint32_t *d_count,
             mk_hit *d_cand, uint64_t *d_rows, const std::function<int(uint32_t, uint32_t)> *after_chunk, uint32_t min_chunks);
int forget_bloom_summary(mk_ctx *c);         // the Bloom cells were replaced: the summaries may claim nothing until recomputed
int ensure_bloom_summary(mk_ctx *c);
int ensure_bloom_summary_arrays(mk_ctx *c);           // allocated and zeroed ("nothing is full"), not computed
uint64_t bloom_summary_bytes(const mk_ctx *c);         // of the coarse level: one bit per 2048 cells
int launch_query_sketch_short(mk_ctx *c, mk_qset *qs);
int launch_query_sketch_long(mk_ctx *c, mk_qset *qs, uint32_t q);
int launch_query_sketch_long_batch(mk_ctx *c, mk_qset *qs, uint32_t q0, uint32_t n, bool *done);
// O(length) sketches of long reads / contigs (per-query hash tables in d_scratch), see sketch.hip
bool query_is_mid_length(const mk_ctx *c, uint64_t nk);
int launch_query_sketch_mid(mk_ctx *c, mk_qset *qs, const std::vector<uint32_t> &which, unsigned long long *d_scratch, uint64_t scratch_slots);
int launch_query_sketch_dense(mk_ctx *c, mk_qset *qs, uint32_t slot);   // slot = index into qs->dense_q
int launch_query_sketch_dense_batch(mk_ctx *c, mk_qset *qs, uint32_t slot, uint32_t n, bool *done);
int launch_scan_counts(mk_ctx *c, mk_qset *qs);                          // fills qs->d_scan_n
// range boundaries of every query's (sorted) entry list; *d_flag |= 1 when a
// (query, range) holds more than `limit` entries
int launch_query_split(mk_ctx *c, mk_qset *qs, uint32_t S, uint32_t limit, uint32_t *d_flag);
int launch_synth_genomes(mk_ctx *c, uint64_t first_id, uint32_t n, uint64_t len, char *d_out);
int launch_synth_queries(mk_ctx *c, uint64_t first_id, uint32_t nq, uint64_t G, uint64_t L, uint64_t qlen,
                         char *d_out);
int launch_convert_columns(mk_ctx *c, bool to_device, uint32_t p_begin, uint32_t p_end, uint8_t *d_staging);
// huff.hip: one lane per deflate block of literals (mk_index_import_columns_huffman)
int launch_huff_decode(mk_ctx *c, const uint8_t *d_payload, uint64_t payload_bytes, const mk_huff_block *d_blocks, uint32_t n_blocks,
                       const uint8_t *d_lens, uint32_t n_codes, uint8_t *d_out, uint64_t out_bytes, uint32_t *d_crc, uint32_t *d_bad);
int launch_export_genomes(mk_ctx *c, const uint32_t *d_ids, uint32_t n, uint8_t *d_dst);   // d_dst[P][n] (W bytes each, dump byte order)
inline MatRef mat_ref(const mk_ctx *c);
// ---- colq.hip: stored columns -> the dense query layout dense[group][p][4] + active counts (slots of 64 at a time:
// consecutive genomes by 16-byte loads, any other list by a byte gather).  A packed index: need_raw_cold first.
uint32_t column_blocks(const mk_ctx *c);                       // partial sums per query
int launch_column_gather(mk_ctx *c, const uint32_t *h_ids, const uint32_t *d_ids, uint32_t nq, uint8_t *d_dense, uint32_t *d_partial,
                         uint32_t *d_nent);
int launch_dense_from_columns(mk_ctx *c, const uint8_t *d_cols, uint32_t nq, uint8_t *d_dense, uint32_t *d_partial, uint32_t *d_nent);

// ---- keep.hip: the genomes ids[0 .. n) (local ids, distinct, below c->G) in that order, in place; raw cold rows; waits for the device
int launch_keep(mk_ctx *c, const uint32_t *ids, uint32_t n);

// ---- extend.hip: src's columns behind dst's in every row (mk_index_extend); dst has the capacity, raw cold rows on both, src's
// stream idle; queued on dst's stream
int launch_extend_place(mk_ctx *dst, const mk_ctx *src);

// ---- gunzip.hip: gzip streams inflated on the device
struct mk_gz_stream {            // a stream (a file) of a batch
    uint64_t in_off;               // its bytes at gz + in_off (16-byte aligned, >= 16 zero bytes behind them)
    uint64_t out_off;              // its text at text + out_off (16-byte aligned)
    uint32_t in_len, n_tok, out_len, status, members;      // status: mk_gz_status
    uint32_t cand_lo, cand_hi;     // its candidate block starts: sorted[cand_lo, cand_hi) (ascending bit offsets)
    uint32_t n_chain;              // segments on its chain: chain[cand_lo + its index ...] (a stream has one more segment than candidates)
    uint32_t rewrite;              // a segment on its chain had more tokens than its slots: those segments are decoded once more, with exact rooms
    uint32_t pad[3];
};
struct mk_gz_seg {                 // what a lane of gz_tokens_kernel found: a stretch of a stream from a block's first bit on
    uint64_t tok_ptr;              // where its tokens lie (a device address, 16-byte aligned)
    uint32_t tok_cap;              // room there (a multiple of four); n_tok > tok_cap: the tokens beyond were counted, not kept
    uint32_t n_tok, out_len, status, members;
    uint32_t link;                 // the segment it arrived at between two blocks (all ones: the stream's end)
};
struct mk_gz_job { uint64_t tok_ptr; uint32_t seg, tok_cap; };   // a segment to decode again, with its exact room
int launch_fasta_count(mk_ctx *c, const uint8_t *d_text, const mk_gz_stream *d_jobs, uint32_t n, const uint32_t *d_chunk_first, uint32_t n_chunks,
                       void *d_scratch, uint64_t *d_seq_len, hipStream_t st);
int launch_fasta_strip(mk_ctx *c, const uint8_t *d_text, const mk_gz_stream *d_jobs, const uint32_t *which, uint32_t m, const uint32_t *h_chunk_first,
                       uint32_t n_chunks, const void *d_scratch, uint8_t *d_dst, const uint64_t *dst_off, hipStream_t st);
uint64_t fasta_scratch_bytes(uint32_t n_chunks);
}  // namespace mk
struct mk_gz_batch;
namespace mk {
int gz_batch_strip(mk_ctx *c, const mk_gz_batch *b, const uint32_t *which, uint32_t m, uint8_t *d_dst, const uint64_t *dst_off, hipStream_t st);
int gz_batch_used(const mk_gz_batch *b, hipStream_t st);       // a kernel that reads the batch's text has been queued on st
uint32_t gz_batch_size(const mk_gz_batch *b);
bool gz_batch_ok(const mk_gz_batch *b, uint32_t i);
uint64_t gz_batch_len(const mk_gz_batch *b, uint32_t i);
const mk_ctx *gz_batch_owner(const mk_gz_batch *b);

// ---- cold.hip: the cold rows packed (delta vs the genome before + bit packing)
int pack_cold(mk_ctx *c, uint64_t *raw_bytes, uint64_t *packed_bytes);
int need_raw_cold(mk_ctx *c);                 // unpack if packed: for everything that needs the rows as they are
int stage_cold_rows(mk_ctx *c, uint64_t r_lo, uint64_t r_hi, uint8_t *d_dst, int b, hipStream_t st);
int ensure_zstage(mk_ctx *c, uint64_t rows);
inline bool has_cold(const mk_ctx *c) { return c->h_M != nullptr || c->h_Z != nullptr; }

// ---- scan.hip
struct ScanArgs {
    const uint8_t *M;
    const uint8_t *Mc;             // cold rows (MatRef::cold_m) or null
    uint32_t P_hot;
    uint64_t ld;
    uint32_t G, ntiles, nq, q_begin;
    const uint64_t *entries;
    const uint64_t *ent_off;
    const uint32_t *nent;
    uint32_t *scores;              // see scan_kernel.hpp: two-stride addressing
    uint64_t score_tile_stride, score_q_stride;
    uint32_t score_vec;            // 16-byte stores allowed (strides and padding permit it)
    // window launches (a matrix with cold rows, scan_windows in api_query.hip): only entries of partitions
    // [row_lo, row_hi) count; accumulate: add to the scores instead of storing them
    uint32_t windowed, row_lo, row_hi, accumulate;
};
int launch_scan(mk_ctx *c, const ScanArgs &a);
// slab schedule: a launch over partition ranges, by the kernel `kind` names (scan_kernel.hpp)
struct SlabArgs {
    const uint8_t *M;
    const uint8_t *Mc;             // cold rows (MatRef::cold_m) or null
    uint32_t P_hot;
    uint32_t r_begin, r_count;     // ranges [r_begin, r_begin + r_count) of the S this launch walks
    uint64_t ld;
    uint32_t G, ntiles, nq, q_begin, S;
    const uint64_t *entries;
    const uint64_t *ent_off;
    const uint32_t *split;         // [query][S + 1] entry indices of the range boundaries
    uint8_t *partials;             // [tile][range][query][1 KiB]
    uint32_t chunk = 0;            // ByCount: range r of a query = its entries [r * chunk, (r + 1) * chunk) instead of the table
    const uint32_t *nent = nullptr;   // ByCount: entries per query
    const uint64_t *lists = nullptr;   // Groups: the query groups' merged lists, groups of kGroupQ
    uint32_t nset = 0;             // queries in the set (the last group may be short)
    // Blocks: the query blocks' lists, blocks of block_q queries of the set
    const uint4 *bpackets = nullptr;
    const BlockInfo *binfo = nullptr;
    uint32_t block_q = 0, range_rows = 0;   // (range r starts at partition r * range_rows)
    // the order of a (tile, range)'s work items: runs of block_sub_fast consecutive sub-tiles vary fastest, then the block,
    // then the runs -- 8 (all of a tile's sub-tiles): sub-tile fastest, 1: block fastest; a divisor of kTileBytes / kBlockTile
    uint32_t block_sub_fast = 8;
    RangedScan kind = RangedScan::PerWave;
};
int launch_scan_slab(mk_ctx *c, const SlabArgs &a);
constexpr uint32_t kGroupQ = 16;         // queries per group of scan_group_kernel
constexpr uint32_t kGroupCells = 2048;   // (window, slot) cells a group's list is ordered by: queries per group x windows per range
int launch_group_lists(mk_ctx *c, mk_qset *qs, uint32_t wshift, uint32_t nwin);
constexpr uint32_t kBlockTile = 128;     // bytes of a row a query block is counted against at a time (scan_block_kernel's T)
constexpr uint32_t kBlockQ = 1280;       // queries per block: kBlockQ x kBlockTile = 160 KiB of LDS counters, all a CU has
static_assert(kBlockQ * kBlockTile <= 160u << 10, "a block's counters fit a CU's LDS");
// SlabArgs::block_sub_fast of a prepared set, unless MIEKKI_SCAN_BLOCK_SUB_FAST says otherwise: block fastest.  Measured at 16, 15
// and 8 blocks per launch and at both fingerprint widths, 9-13 % faster than 8 everywhere (profiles/r13_scan_block_order.txt),
// so it is one value and no function of the launch's blocks.
constexpr uint32_t kBlockSubFast = 1;
// blocks per launch that a caller who asks for several chunks (for_chunks' min_chunks: the exchange of a sharded run) still gets:
// block fastest, sixteen blocks are a round of an XCD's 32 CUs on two sub-tiles, the default chunk of the large sets
constexpr uint32_t kBlockShareBlocks = 16;
// A list is padded with ZERO packets (row 0 of the range, no pairs) to whole steps of scan_block_kernel: 128 lane groups x 4
// packets at kBlockTile.  List (block, range) begins (block x S + range) x kBlockStepPackets packets behind the room its
// queries' entries have, so every list has its padding to itself (qset_block_lists sizes the buffer for it).
constexpr uint32_t kBlockStepPackets = 512;
// the order of a step's requests in scan_block_kernel (scan_kernel.hpp); B measured 10 % faster than A
// (profiles/r15_scan_block_ab.txt)
constexpr int kOrderA = 0, kOrderB = 1;
constexpr int kBlockOrder = kOrderB;
int launch_block_lists(mk_ctx *c, mk_qset *qs);
// the two layouts the pipeline uses
struct ScoreLayout { uint64_t tile_stride, q_stride; uint32_t vec; };
inline ScoreLayout score_layout_rows(uint32_t W, uint64_t pitch, uint32_t G)      // [query][pitch]
{
    const uint64_t tg = kTileBytes / W;
    return {tg, pitch, (uint32_t)((pitch % 4 == 0) && ((uint64_t)((G + tg - 1) / tg) * tg <= pitch))};
}
inline ScoreLayout score_layout_tiles(uint32_t W, uint32_t nq)                     // [tile][query][genomes per tile]
{
    const uint64_t tg = kTileBytes / W;
    return {(uint64_t)nq * tg, tg, 1u};
}

// dense long queries (scan_kernel.hpp: scan_dense_kernel): adds into the score rows
struct DenseLut;
struct DenseArgs {
    const uint8_t *M;
    const uint8_t *Mc;             // cold rows (MatRef::cold_m) or null
    uint32_t P_hot;
    uint64_t ld;
    uint32_t G, ntiles, P, rows_per_item, nchunks, ngroups;
    uint32_t row_lo, row_hi;       // rows this launch walks (nchunks covers them in pieces of rows_per_item)
    const uint8_t *dense;          // [group][P][4] fingerprints (W bytes each), empty = inactive
    const uint32_t *dense_q;       // [group][4] set index of each slot or 0xffffffff
    const DenseLut *lut;    // one-byte fingerprints: [octet = two groups][P] field tables (scan_kernel.hpp), or null
    uint32_t noctets;
    uint32_t q0, q1;               // set range the score buffer covers
    uint32_t *scores;
    uint64_t score_tile_stride, score_q_stride;
    uint32_t empty;
};
int launch_scan_dense(mk_ctx *c, const DenseArgs &a);
int launch_dense_lut(mk_ctx *c, const uint8_t *d_dense, uint32_t ngroups, DenseLut *d_lut);
// how the table kernel shares rows between its sets of queries (scan.hip, scan_kernel.hpp): sets of sixteen (eight) queries,
// sharing groups of 1, 2 or 4 sets -- and the rows a chunk may hold for the counters' bit planes
inline uint32_t dense_share(uint32_t noctets) { const uint32_t no = noctets >= 2 ? 2 : 1, nsets = (noctets + no - 1) / no; return nsets >= 3 ? 4u : nsets == 2 ? 2u : 1u; }
inline uint32_t dense_chunk_rows(uint32_t noctets) { (void)noctets; return 16368u; }
int probe_stream_read(mk_ctx *c, uint32_t rounds, double *gbps, uint64_t *bytes);
int probe_ne_lanes(mk_ctx *c, uint32_t W, const uint32_t *d, const uint32_t *b, uint64_t n, uint32_t *flags);

// ---- a scanned chunk of a query set, as everything behind the scan reads it (api_query.hip: chunk_view fills it)
struct ChunkView {
    const uint32_t *scores;        // tile-major [tile][nq][tile_genomes] (plain schedule) or null
    const uint8_t *partials;       // [tile][range][nq][1 KiB] mismatch counts (slab schedule) or null
    const uint32_t *nent;          // active partitions per query, offset to this chunk (slab schedule) or null
    uint32_t S, W;
    uint32_t tile_genomes, G;
    uint32_t nq;                   // queries of the chunk: the strides of scores / partials
    uint32_t min_score;
    double min_inter;
    const uint32_t *sketch_size;
    const uint64_t *genome_size;
    uint32_t genome_id_base;
    const float *ratio;            // genome_size / sketch_size per genome (slab schedule: the screen's one load), or null
};

// ---- select.hip
struct SelectArgs {
    ChunkView v;
    uint32_t nresults, cap;
    uint32_t *count;               // [nq]
    mk_hit *cand;                  // [nq][cap]
    uint64_t *rows;                // compact form instead of count/cand: [nq][1 + cap], see mk_qset_run_compact
};
constexpr uint32_t kSelectMaxResults = 64;   // top-N sizes the device selection supports
int launch_select(mk_ctx *c, const SelectArgs &a);
int launch_ratio(mk_ctx *c, float *d_ratio, uint32_t padded);

// ---- merge.hip (K6b): filter_results' heap over the entrant rows of `world` shards
constexpr uint32_t kMergeOverflow = 0xffffffffu;   // nhits value of a query some shard's row overflowed for
struct MergeArgs {
    const uint32_t *count;         // [world][nq]
    const mk_hit *cand;            // [world][nq][cap]
    uint32_t world, nq, cap, nresults;
    mk_hit *hits;                  // [nq][nresults]
    uint32_t *nhits;               // [nq]
    // compact exchange form instead of count / cand (null otherwise): [world][nq][1 + cap] words
    const uint64_t *rows;
    const uint32_t *ss;            // sketch_size of every genome a row may name, indexed by id - id_base
    const uint64_t *gs;            // genome_size likewise
    uint32_t id_base;
};
int launch_merge(mk_ctx *c, const MergeArgs &a);

// ---- list.hip: every genome above the thresholds (filter_results with nresults beyond the device selection's 64)
// (the walk's kernels keep the chunk's fields flat among their own: list_kernel's scalar registers follow the struct;
// api_query.hip: list_args copies them from the ChunkView)
struct ListArgs {
    const uint32_t *scores;        // as SelectArgs: tile-major u32 scores ...
    const uint8_t *partials;       // ... or the slab schedule's per-range mismatch counts
    const uint32_t *nent;          // active partitions per query of the chunk (slab schedule)
    uint32_t S, W;
    uint32_t tile_genomes, G;
    uint32_t nq;                   // queries of the chunk the scores / partials were written for (their strides)
    uint32_t q_lo, q_n;            // queries [q_lo, q_lo + q_n) of the chunk are this launch's
    uint32_t min_score;
    double min_inter;
    const uint32_t *sketch_size;
    const uint64_t *genome_size;
    uint32_t genome_id_base;
    const float *ratio;            // slab schedule: the screen's one float per genome
    uint32_t *count;               // count pass: [nq] passing genomes per query
    const uint64_t *rec_off;       // write pass: [nq + 1] exclusive scan of count; query q's records start at rec[rec_off[q] - rec_off[q_lo]]
    uint64_t *rec;                 // genome | matches << 32, ascending genome id per query
};
int launch_list_count(mk_ctx *c, const ListArgs &a);
int launch_list_write(mk_ctx *c, const ListArgs &a);
// rec_off[n + 1] = exclusive scan of count, res_off[n + 1] = exclusive scan of min(count, nresults)
int launch_list_scan(mk_ctx *c, const uint32_t *d_count, uint32_t n, uint32_t nresults, uint64_t *d_rec_off, uint64_t *d_res_off);
struct ListHeapArgs {
    const uint64_t *rec;
    const uint64_t *rec_off, *res_off;   // [nq + 1] of the chunk
    uint32_t q_lo, q_n;
    uint32_t nresults;
    const uint32_t *sketch_size;   // of this context's genomes, indexed by id - id_base
    const uint64_t *genome_size;
    uint32_t id_base;
    double *key;                   // the heaps: query q's min(nresults, count) + 1 entries at res_off[q] - res_off[q_lo] + (q - q_lo)
    uint32_t *ref;
    mk_hit *hits;                  // query q's hits at res_off[q] - res_off[q_lo]
};
int launch_list_heap(mk_ctx *c, const ListHeapArgs &a);
// records -> hits in the records' own order (the candidates a sharded run concatenates): hits[i] from rec[i]
int launch_list_expand(mk_ctx *c, const uint64_t *d_rec, uint64_t n, const uint32_t *ss, const uint64_t *gs, uint32_t id_base, mk_hit *d_hits);

// ---- family.hip: the list walk with a union-find forest as its sink (api_sinks.hip: mk_qset_run_link, mk_index_families)
struct LinkArgs {
    ListArgs list;                 // the chunk, as for the lists (count, rec_off, rec unused)
    const uint32_t *query_ids;     // [list.nq] the id each query of the chunk stands for
    uint32_t *parent;              // the forest: every query id and every genome id of the context is below its size
};
int launch_link(mk_ctx *c, const LinkArgs &a);
// the same walk at levels[0]'s thresholds (list.min_score, list.min_inter are those), every passing pair joined in the forest
// of the strictest level it passes (api_sinks.hip: mk_qset_run_link_levels, mk_index_hierarchy)
struct LinkLevelsArgs {
    LinkArgs link;                 // link.parent: n_levels forests one after the other, [n_levels][n_ids]
    uint32_t n_levels, n_ids;
    mk_level levels[MK_MAX_LEVELS];
};
int launch_link_levels(mk_ctx *c, const LinkLevelsArgs &a);
int launch_link_reset(mk_ctx *c, uint32_t *d_parent, uint32_t n);
int launch_link_merge(mk_ctx *c, uint32_t *d_parent, const uint32_t *d_other, uint32_t n);
int launch_link_labels(mk_ctx *c, const uint32_t *d_parent, uint32_t n, uint32_t *d_label);

// ---- the counting sinks on the list walk: tally.hip, clade.hip, lca.hip (their shared device pieces: walk_best.hpp).  Counters
// of any of them start as zeros, queued on c->stream: the body of mk_tally_reset, mk_clade_tally_reset and mk_lca_tally_reset.
template <typename T>
inline int counters_reset(mk_ctx *c, T *d, uint32_t n)
{
    if (!c || (n && !d)) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (n) MK_HIP(hipMemsetAsync(d, 0, (size_t)n * sizeof(T), c->stream));
    return MK_OK;
}

// ---- tally.hip: the list walk with four counters per genome as its sink (mk_qset_run_tally, mk_query_tally)
struct TallyArgs {
    ListArgs list;                 // the chunk, as for the lists (count, rec_off, rec unused)
    mk_tally *tally;               // [list.G] the counters of the context's own genomes: the caller's array + genome_id_base
};
int launch_tally(mk_ctx *c, const TallyArgs &a);

// ---- clade.hip: the list walk with five counters per clade of genomes as its sink (mk_qset_run_clade_tally, mk_query_clade_tally)
struct CladeArgs {
    ListArgs list;                 // the chunk, as for the lists (count, rec_off, rec unused)
    const uint32_t *clade;         // [map_n] clade number per local genome, non-decreasing among those that have one; MK_NO_CLADE: left out
    uint32_t map_n;                // entries of `clade`, whole tiles of kTileBytes genomes: genomes from map_n on are left out
    mk_clade_tally *tally;         // the counters: every clade number of the map is below their size
};
int launch_clade_tally(mk_ctx *c, const CladeArgs &a);

// ---- lca.hip: the list walk with three counters per node of a taxonomy as its sink (mk_qset_run_lca, mk_query_lca)
struct LcaArgs {
    ListArgs list;                 // the chunk, as for the lists (count, rec_off, rec unused)
    const uint32_t *leaf;          // [map_n] the deepest node that holds each local genome; MK_NO_NODE: left out
    uint32_t map_n;                // entries of `leaf`, whole tiles of kTileBytes genomes: genomes from map_n on are left out
    const uint32_t *parent;        // [n_nodes] the smallest enclosing node, MK_NO_NODE for a root
    const uint32_t *hi;            // [n_nodes] one past the node's last genome
    uint32_t n_nodes, depth;       // depth: the largest number of ancestors any node has -- a climb ends within depth + 1 steps
    uint32_t margin;               // 0 .. 100
    mk_lca_tally *tally;           // [n_nodes + 1] the counters, the last slot for "above every node"
    uint32_t *node;                // null, or the set's per-query nodes: query q0 + i of the leaf writes node[place ? place[q0 + i] : q0 + i]
    const uint32_t *place;         // null, or [leaf's queries] their places in the set (a part of a mixed set)
    uint32_t q0;                   // the place in the leaf of the chunk's first query
};
int launch_lca(mk_ctx *c, const LcaArgs &a);

// ---- share.hip: the list walk with a pool of per-read genome lists as its sink, and the EM rounds over the pool
// (mk_qset_run_share, mk_share_add_lists, mk_share_rounds).  Ids are local genome numbers.
struct ShareArgs {
    ListArgs list;                 // the chunk; count[q] = |K(q)| of a shared query, else 0; rec_off = the exclusive scan of count
    uint32_t margin;               // 0 .. 100
    double *least;                 // [list.nq] x* (100 - margin) of the queries the second walk counted
    const uint64_t *read_off;      // write pass: [list.nq + 1] the exclusive scan of min(count, 1): a shared query's place among the chunk's lists
    uint64_t *unique, *shared;     // [list.G] the pool's counters
    uint64_t *settled;             // one word: the chunk's settled queries are added to it
    uint32_t *ids;                 // write pass: the pool's ids and offsets, with room for the chunk's
    uint64_t *off;
    uint64_t entries0, reads0;     // ids and lists the pool held before the chunk
};
int launch_share_count(mk_ctx *c, const ShareArgs &k);
int launch_share_write(mk_ctx *c, const ShareArgs &k);
int launch_share_bump(mk_ctx *c, const uint32_t *d_ids, uint64_t n, uint64_t *d_counters);   // d_counters[d_ids[i]] += 1
struct RoundArgs {
    const uint32_t *ids;           // the pool
    const uint64_t *off;
    uint64_t n_reads;
    const uint64_t *prev;          // [G] the sums of the round before, or null: round 1, every weight 1
    uint64_t *next;                // [G] this round's sums, seeded with unique << 32
    uint32_t shift;
    uint64_t *starved;             // null, or the word that counts the reads whose weights sum to zero
};
int share_team(uint32_t *team);    // lanes per read of the round kernel: 16, or MIEKKI_SHARE_TEAM checked: MK_ERR_ARG before any launch
int launch_share_seed(mk_ctx *c, const uint64_t *d_unique, uint32_t G, uint64_t *d_next);
int launch_share_round(mk_ctx *c, const RoundArgs &k, uint32_t team);
int launch_share_delta(mk_ctx *c, const uint64_t *d_now, const uint64_t *d_before, uint32_t G, uint64_t *d_delta);   // *d_delta is added to

// ---- cover.hip: a set's gated sketch as bits of a (partition, value) table, and the per-genome counts of one pass over the
// matrix (mk_qset_run_cover, mk_cover_count, mk_query_cover); the mark walks and the pass are table_pass.hpp's, which depth.hip
// shares.  Everything is queued on c->stream.
uint64_t cover_table_bytes(const mk_ctx *c);                                      // P << fp_bits >> 3
int launch_cover_reset(mk_ctx *c, uint32_t *d_seen);
int launch_cover_mark(mk_ctx *c, const mk_qset *qs, uint32_t *d_seen);            // a sketched set that is not a shell over parts
// d_covered[G] and *d_cells are added to (either may be null): the caller zeroes them; raw cold rows
int launch_cover_count(mk_ctx *c, const uint32_t *d_seen, uint32_t *d_covered, unsigned long long *d_cells);
// the winner-takes-all pass (mk_cover_assign): d_won[G] is added to; d_rank[G], 0 = best, and d_order[G], its inverse; raw cold rows
int cover_win_values(const mk_ctx *c, uint32_t *values);                          // MIEKKI_WIN_VALUES checked: MK_ERR_ARG before any launch
int launch_cover_win(mk_ctx *c, const uint32_t *d_seen, const uint32_t *d_rank, const uint32_t *d_order, uint32_t *d_won);

// ---- taxcover.hip: per node of a taxonomy the distinct cells its genomes hold and those of them a cover table has seen
// (mk_taxonomy_cover).  A work item is a node and a chunk of rows, a wave's; sub: 64 for a wide node, for a narrow one the
// lanes that take a row (one byte) or 0 (two bytes).
struct TaxItem { uint32_t node, r_lo, r_hi, sub; };
int taxcover_switches(const mk_ctx *c, uint32_t *rows, uint32_t *wide);            // MIEKKI_TAXCOVER_ROWS / _WIDE checked: MK_ERR_ARG before any launch
// the items of the nodes of width >= 2; rows: the switch's, 0 = by width
int taxcover_items(const mk_ctx *c, const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes, uint32_t rows, uint32_t wide, std::vector<TaxItem> &items);
// d_out[node] is added to: the caller zeroes it; d_seen may be null; raw cold rows
int launch_taxcover(mk_ctx *c, const TaxItem *d_items, uint32_t n_items, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_seen,
                    mk_node_cover *d_out);

// ---- markers.hip: every held cell credited to the deepest node of a taxonomy that contains all its holders, and those of a
// node's own cells a cover table has seen (mk_taxonomy_markers).  One pass in the shape of the win pass.
int markers_switches(const mk_ctx *c, uint32_t *rows, uint32_t *values, uint32_t *flags);   // MIEKKI_MARK_* checked: MK_ERR_ARG before any launch
// d_out[n_nodes + 1] is added to: the caller zeroes it; d_seen may be null; d_live: a bit per genome, whole tiles, 0 from n on;
// raw cold rows
int launch_markers(mk_ctx *c, const uint32_t *d_leaf, const uint32_t *d_parent, const uint32_t *d_hi, const uint32_t *d_live, uint32_t n,
                   uint32_t n_nodes, const uint32_t *d_seen, mk_node_markers *d_out);

// ---- depth.hip: a set's gated sketch as saturating byte counters of a (partition, value) table, and per genome the covered
// fingerprints, the sum and the median of their counters (mk_qset_run_depth, mk_depth_profile, mk_query_depth), by
// table_pass.hpp's walks and pass with a byte for a cell.  Everything is queued on c->stream.
uint64_t depth_table_bytes(const mk_ctx *c);                                      // P << fp_bits
int launch_depth_reset(mk_ctx *c, uint8_t *d_mult);
int launch_depth_mark(mk_ctx *c, const mk_qset *qs, uint8_t *d_mult);             // a sketched set that is not a shell over parts
uint64_t depth_scratch_words(uint32_t G);                                         // 32-bit words of launch_depth_profile's scratch
// d_out[G] is written after pass 0 and the 8 bisection passes; d_scratch at an 8-byte boundary; raw cold rows
int launch_depth_profile(mk_ctx *c, const uint8_t *d_mult, uint32_t *d_scratch, mk_depth *d_out);
int launch_depth_cells(mk_ctx *c, const uint8_t *d_mult, unsigned long long *d_totals);   // [cells, saturated] are added to

// ---- panel.hip: up to eight samples' gated sketches as the bits of a (partition, value) table of bytes, and the per-slot,
// per-genome counts of ONE pass over the matrix (mk_qset_run_panel, mk_panel_count, mk_panel_slot, mk_query_panel): table_pass.hpp's
// walks, a pass of its own that counts mask words in bit planes.  Everything is queued on c->stream.
uint64_t panel_table_bytes(const mk_ctx *c);                                      // P << fp_bits
int launch_panel_reset(mk_ctx *c, uint8_t *d_panel);
int launch_panel_mark(mk_ctx *c, const mk_qset *qs, uint32_t slot, uint8_t *d_panel);     // a sketched set that is not a shell over parts; slot < 8
// d_covered[n_slots][G] and d_cells[8] are added to (either may be null): the caller zeroes them; raw cold rows
int launch_panel_count(mk_ctx *c, const uint8_t *d_panel, uint32_t n_slots, uint32_t *d_covered, unsigned long long *d_cells);
int launch_panel_slot(mk_ctx *c, const uint8_t *d_panel, uint32_t slot, uint32_t *d_seen);   // d_seen (cover_table_bytes) is written

// ---- gather.hip: the greedy set cover over a cover table (mk_cover_gather): a round = pick + take + strike (or recount), queued
// on c->stream; raw cold rows
struct GatherArgs {
    uint32_t *live;                // the call's own copy of the cover table: struck cells are cleared
    const uint8_t *mult;           // the caller's depth table or null
    uint32_t *rem;                 // [G] what every genome still explains
    unsigned long long *slots;     // [rounds] the rounds' arg-max keys, zeroed
    mk_pick *recs;                 // [rounds] the pick records, zeroed: genome (local id), fresh, covered = the strike list's length, depth_sum
    uint64_t *list;                // [P] the strike list of the round in flight: p | v << 32
    uint32_t *done;                // one word, zeroed: set by the take step of the round that stops the loop
    uint32_t min_new, cap;         // cap: rounds at the most
    bool recount;
};
bool gather_recount();             // MIEKKI_GATHER_RECOUNT
uint32_t gather_rounds_per_wait(); // MIEKKI_GATHER_ROUNDS
int launch_gather_round(mk_ctx *c, const GatherArgs &a, uint32_t round);

// ---- rep.hip: the list walk with a bitmap row per query as its sink, and greedy representatives over the rows
// (mk_index_representatives).  Ids are local genome numbers.
constexpr uint32_t kRepMaxSet = 1024;   // ids per resolve step: their n x n link matrix is 128 KiB of the workgroup's 160 KiB of LDS
struct RepRowsArgs {
    ListArgs list;                 // the chunk, as for the lists (count, rec_off, rec unused): u32 scores
    uint32_t chunk_pos;            // the place in the set of the chunk's first query
    uint32_t set_g0;               // the genome the set's first query is: the query at place p is genome set_g0 + p
    uint32_t *rows;                // [set][row_words]: bit g of row p = the query at place p lists genome g
    uint32_t row_words;            // >= rep_row_words(G): whole steps of the walk
};
struct RepArgs {
    const uint32_t *rows;          // the rows of genomes [set_g0, set_g0 + n), complete
    uint32_t row_words;
    uint32_t set_g0, n;            // the ids to resolve: a set, or a piece of one; n <= kRepMaxSet
    uint32_t G;
    uint32_t *rep;                 // [G]
    uint32_t *is_rep;              // [(G + 31) / 32]: the representatives among the genomes below the set
};
uint32_t rep_row_words(uint32_t G);
int launch_rep_rows(mk_ctx *c, const RepRowsArgs &a);
int launch_rep_reset(mk_ctx *c, uint32_t *d_rep, uint32_t n, uint32_t *d_is_rep);
int launch_rep_resolve(mk_ctx *c, const RepArgs &a);       // below + resolve + propagate of one set, queued behind its rows

// ---- api_query.hip, for the sinks of api_sinks.hip: a sink's pass over a set is qset_leaves + qset_walk, a loop over a caller's
// sequences for_uploaded_slices, a loop of the index over itself for_index_sets (index_set_ids ids per set)
void qset_release(mk_qset *qs);
int qset_sketch_only(mk_ctx *c, mk_qset *qs);          // the sketch without the slab tables
int refuse_nan_lists(mk_ctx *c, uint32_t min_score);   // MK_ERR_UNSUPPORTED where a NaN intersection could be listed
int qset_leaves(mk_ctx *c, mk_qset *qs, const std::function<int(mk_qset *leaf, const std::vector<uint32_t> *places)> &fn);
int qset_walk(mk_ctx *c, mk_qset *leaf, uint32_t min_score, double min_inter, const std::function<int(uint32_t q0, const ListArgs &)> &sink);
int for_uploaded_slices(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, const std::function<int(mk_qset *qs, uint32_t q0, uint32_t n)> &fn);
uint32_t index_set_ids(const mk_ctx *c);
int for_index_sets(mk_ctx *c, uint32_t per, const std::function<int(mk_qset *qs, const uint32_t *ids, uint32_t g0, uint32_t n)> &fn);

// ---- exact.hip
int exact_load_genome(mk_ctx *c, const char *const *contigs, const uint64_t *contig_lens, uint32_t n_contigs);
int exact_queries(mk_ctx *c, const char *const *queries, const uint64_t *query_lens, uint32_t nq, uint64_t *inter,
                  uint64_t *uni);

}  // namespace mk
