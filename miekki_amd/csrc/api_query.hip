// C ABI of libmiekki_hip.so, the query side: query sets (sketch, Bloom gate, range tables), the scan schedules (slab, plain,
// dense, windows over rows in host memory), selection, and mk_query / mk_query_scores / mk_qset_* / mk_exact* above them.
// Host-side orchestration only: the kernels are in sketch.hip, colq.hip, scan.hip, select.hip, merge.hip, list.hip, exact.hip.
// Every pass over a set -- selection, mk_query, lists, the walks of api_sinks.hip's sinks -- is a body of ONE chunk loop (for_chunks).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>

#include "mk_internal.hpp"

namespace mk {

// A genome without a single stored fingerprint (its sequence is exactly k long, Miekki.cpp:162,
// 569) has sketch_size 0: with min_score 0 its score 0 passes and jaccard = 0 / 0 is NaN
// (Miekki.cpp:381-383).  What the reference's heap does with NaNs is whatever its comparison
// sequence happens to yield; the device selection assumes ordered values, so such calls take
// the host replay (dense score rows + the same std:: heap calls), which reproduces it.
static bool nan_candidates_possible(const mk_ctx *c, uint32_t min_score)
{
    return min_score == 0 && c->has_empty_sketch;
}

// ---- query sets ------------------------------------------------------------------
// rows of a part of a mixed set to their places in the whole set's output: row i -> dst[idx[i]] (row_bytes a multiple of 8),
// and, when there are separate counts, cnt[i] -> dst_cnt[idx[i]]
__global__ __launch_bounds__(256) void place_rows_kernel(const uint8_t *__restrict__ rows, uint64_t row_bytes, const uint32_t *__restrict__ idx, uint32_t n,
                                                         uint8_t *__restrict__ dst, const uint32_t *__restrict__ cnt, uint32_t *__restrict__ dst_cnt)
{
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const uint32_t q = idx[i];
    const uint64_t *__restrict__ s = reinterpret_cast<const uint64_t *>(rows + (uint64_t)i * row_bytes);
    uint64_t *__restrict__ d = reinterpret_cast<uint64_t *>(dst + (uint64_t)q * row_bytes);
    // (a count form's row is only as full as its count says -- 24 bytes per hit -- but copying the slots is cheaper than asking)
    for (uint64_t w = threadIdx.x; w < row_bytes / 8; w += blockDim.x) d[w] = s[w];
    if (cnt && threadIdx.x == 0) dst_cnt[q] = cnt[i];
}

static int launch_place_rows(mk_ctx *c, const uint8_t *rows, uint64_t row_bytes, const uint32_t *d_idx, uint32_t n, uint8_t *dst, const uint32_t *cnt,
                             uint32_t *dst_cnt)
{
    if (!n) return MK_OK;
    hipLaunchKernelGGL(place_rows_kernel, dim3(n), dim3(256), 0, c->stream, rows, row_bytes, d_idx, n, dst, cnt, dst_cnt);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

void qset_release(mk_qset *qs)
{
    if (!qs) return;
    for (int i = 0; i < 2; ++i) { qset_release(qs->part[i]); dev_free(qs->d_part_q[i]); }
    dev_free(qs->d_part_out);
    if (!qs->split_in_arena) dev_free(qs->d_split);
    dev_free(qs->d_glist);
    dev_free(qs->d_bpackets); dev_free(qs->d_binfo);
    if (qs->arena_borrowed) qs->owner->qarena_busy = false;      // the context keeps its arena for the next call
    else dev_free(qs->d_arena);                  // every other device array of the set lives in it
    delete qs;
}

// lens == null: a set made from stored columns (colq.hip) -- every query dense, no sequences
// cuts != null: a set of read pairs -- lens[q] = both mates' characters, cuts[q] = mate 1's; a pair counts the k-mers of
// its mates, each on its own, and is always short (mk_qset_upload_pairs has refused the others)
// masked: a set with base qualities (mk_qset_upload_reads), pairs or not -- a key slot per window of the query's characters,
// lens[q] - k of them, and always short (the call has refused the others); room for the qualities beside the sequences
static int qset_alloc(mk_ctx *c, const uint64_t *lens, uint32_t nq, mk_qset **out, bool transient = false, const uint32_t *cuts = nullptr,
                      bool masked = false)
{
    std::unique_ptr<mk_qset, void (*)(mk_qset *)> qs(new mk_qset(), qset_release);
    qs->owner = c; qs->nq = nq;
    qs->columns = lens == nullptr;
    qs->h_off.assign(nq + 1, 0); qs->h_ent_off.assign(nq + 1, 0);
    // Long queries that activate a large share of the partitions (whole genomes, -A) keep a dense fingerprint vector
    // instead of an entry list and are scored by passes over ALL rows, sixteen queries per pass (scan_dense_lut_kernel).  From
    // which share on that is cheaper depends on how many there are to share a pass: a pass costs what 16 x 0.115 P entries cost
    // the sparse scan (27.7 ms per 105 GB against 7.1 TB/s of entries), i.e. a query with more than P / 8 k-mers (0.118 P
    // active partitions) is better off dense when a pass is full, and one with P / 4 (0.22 P) even when it has a pass nearly
    // to itself.  (The vectors and tables of the dense queries stay below 8 GiB.)
    uint64_t dense_div = 4;
    if (lens && !cuts && !masked) {
        uint64_t n8 = 0;
        for (uint32_t q = 0; q < nq; ++q) {
            const uint64_t nk = lens[q] > c->p.k ? lens[q] - c->p.k : 0;
            n8 += beyond_short_len(c->p.k, lens[q]) && nk >= c->P / 8 ? 1 : 0;
        }
        if (n8 >= 16 && n8 * c->P * c->W * 3 <= (8ull << 30)) dense_div = 8;       // (vector: P W bytes per query; tables: 2 P W per query)
    }
    for (uint32_t q = 0; q < nq; ++q) {
        if (!lens) { qs->dense_q.push_back(q); continue; }
        if (cuts || masked) {
            const uint64_t nk = masked ? (lens[q] > c->p.k ? lens[q] - c->p.k : 0) : pair_kmers(c->p.k, cuts[q], lens[q] - cuts[q]);
            qs->h_off[q + 1] = qs->h_off[q] + lens[q];
            qs->h_ent_off[q + 1] = qs->h_ent_off[q] + std::min<uint64_t>(nk, c->P);
            qs->short_max_nk = std::max<uint32_t>(qs->short_max_nk, (uint32_t)nk);
            continue;
        }
        const uint64_t nk = lens[q] > c->p.k ? lens[q] - c->p.k : 0;
        if (lens[q] >= (1ull << 40)) { set_error("query too long"); return MK_ERR_ARG; }
        qs->h_off[q + 1] = qs->h_off[q] + lens[q];
        const bool dense = beyond_short_len(c->p.k, lens[q]) && nk >= c->P / dense_div;
        qs->h_ent_off[q + 1] = qs->h_ent_off[q] + (dense ? 0 : std::min<uint64_t>(nk, c->P));
        if (dense) qs->dense_q.push_back(q);
        else if (beyond_short_len(c->p.k, lens[q])) qs->long_q.push_back(q);
        else qs->short_max_nk = std::max<uint32_t>(qs->short_max_nk, (uint32_t)nk);
    }
    qs->total_len = qs->h_off[nq];
    // One device allocation per set (a small call is dominated by allocator round trips, not by
    // kernels): the arrays are carved out of it at 256-byte boundaries.
    uint64_t dense_bytes = 0;
    if (!qs->dense_q.empty()) {
        while (qs->dense_q.size() % 4) qs->dense_q.push_back(0xffffffffu);          // pad the last group
        dense_bytes = (uint64_t)(qs->dense_q.size() / 4) * c->P * 4 * c->W;
    }
    constexpr uint32_t kSplitS = 32;                                // room for the slab schedule's range table up to S = 32
    qs->split_room = (uint64_t)nq * (kSplitS + 1) * 4 <= (64ull << 20) ? kSplitS : 0;
    uint64_t at = 0;
    auto carve = [&at](uint64_t bytes) { const uint64_t o = at; at += (bytes + 255) / 256 * 256; return o; };
    const uint64_t o_seq = carve(qs->total_len + 64), o_off = carve(((uint64_t)nq + 1) * 8),
                   o_ent_off = carve(((uint64_t)nq + 1) * 8), o_entries = carve((qs->h_ent_off[nq] + 1) * 8),
                   o_nent = carve(((uint64_t)nq + 1) * 4), o_scan_n = carve(((uint64_t)nq + 1) * 4),
                   o_dense = carve(dense_bytes), o_dense_q = carve(qs->dense_q.size() * 4),
                   o_lut = carve((uint64_t)((qs->dense_q.size() / 4 + 1) / 2) * c->P * 32),     // (32 bytes of tables per octet of queries and row, either width)
                   o_split = carve(qs->split_room ? (uint64_t)nq * (qs->split_room + 1) * 4 : 0),
                   o_col_ids = carve(qs->columns ? (uint64_t)nq * 4 : 0),
                   o_col_partial = carve(qs->columns ? (uint64_t)nq * column_blocks(c) * 4 : 0),
                   o_cut = carve(cuts ? (uint64_t)nq * 4 : 0), o_qual = carve(masked ? qs->total_len + 64 : 0);
    if (transient && !c->qarena_busy) {
        if (at > c->d_qarena.cap) {
            MK_HIP(hipStreamSynchronize(c->stream));
            MK_TRY(c->d_qarena.alloc(std::max<uint64_t>(at + at / 2, 4ull << 20)));
        }
        qs->d_arena = c->d_qarena; qs->arena_borrowed = true; c->qarena_busy = true;
    } else {
        MK_TRY(dev_alloc(&qs->d_arena, at));
    }
    qs->o_off = o_off; qs->o_ent_off = o_ent_off;
    qs->head_bytes = o_ent_off + ((uint64_t)nq + 1) * 8;          // o_seq == 0: sequences, offsets, entry offsets in a row
    qs->d_seq = reinterpret_cast<char *>(qs->d_arena + o_seq);
    qs->d_off = reinterpret_cast<uint64_t *>(qs->d_arena + o_off);
    qs->d_ent_off = reinterpret_cast<uint64_t *>(qs->d_arena + o_ent_off);
    qs->d_entries = reinterpret_cast<uint64_t *>(qs->d_arena + o_entries);
    qs->d_nent = reinterpret_cast<uint32_t *>(qs->d_arena + o_nent);
    qs->d_scan_n = reinterpret_cast<uint32_t *>(qs->d_arena + o_scan_n);
    if (qs->split_room) { qs->d_split = reinterpret_cast<uint32_t *>(qs->d_arena + o_split); qs->split_in_arena = true; }
    if (cuts) qs->d_cut = reinterpret_cast<uint32_t *>(qs->d_arena + o_cut);
    if (masked) qs->d_qual = qs->d_arena + o_qual;
    if (qs->columns) {
        qs->d_col_ids = reinterpret_cast<uint32_t *>(qs->d_arena + o_col_ids);
        qs->d_col_partial = reinterpret_cast<uint32_t *>(qs->d_arena + o_col_partial);
    }
    if (!qs->dense_q.empty()) {
        qs->d_dense = qs->d_arena + o_dense;
        qs->d_dense_q = reinterpret_cast<uint32_t *>(qs->d_arena + o_dense_q);
        qs->d_dense_lut = reinterpret_cast<DenseLut *>(qs->d_arena + o_lut);
        MK_HIP(hipMemsetAsync(qs->d_dense, 0xFF, dense_bytes, c->stream));           // every slot starts empty
        MK_HIP(hipMemcpyAsync(qs->d_dense_q, qs->dense_q.data(), qs->dense_q.size() * 4, hipMemcpyHostToDevice,
                              c->stream));
    }
    *out = qs.release();                                         // offsets travel with the sequences (qset_upload)
    return MK_OK;
}

static int qset_copy_offsets(mk_ctx *c, mk_qset *qs)
{
    MK_HIP(hipMemcpyAsync(qs->d_off, qs->h_off.data(), (size_t)(qs->nq + 1) * 8, hipMemcpyHostToDevice, c->stream));
    MK_HIP(hipMemcpyAsync(qs->d_ent_off, qs->h_ent_off.data(), (size_t)(qs->nq + 1) * 8, hipMemcpyHostToDevice,
                          c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));                     // the host vectors are pageable
    return MK_OK;
}

static int ensure_pinned(PinnedArray<uint8_t> &h, uint64_t need)
{
    return need <= h.cap ? MK_OK : h.alloc(std::max<uint64_t>(need + need / 2, 1ull << 20));
}

static int qset_prepare_slab(mk_ctx *c, mk_qset *qs);

// the "sketch" of a set made from stored columns: the gather of its genomes' columns as the index holds them now (a
// set made from a caller's columns keeps what it was made with), the field tables, the scan counts
static int qset_sketch_columns(mk_ctx *c, mk_qset *qs)
{
    if (qs->from_index) {
        if (qs->index_id != c->index_id) { set_error("the query set was made from the index before its genomes were selected or replaced: its ids name other genomes now"); return MK_ERR_STATE; }
        for (uint32_t g : qs->col_ids)
            if (g >= c->G) { set_error("the query set names genome %u, which the index no longer holds", g + c->p.genome_id_base); return MK_ERR_STATE; }
        MK_TRY(need_raw_cold(c));                                  // (the rule the exports follow: packed cold rows are unpacked first)
    }
    ScopedTimer t(c, 0);
    if (qs->from_index) MK_TRY(launch_column_gather(c, qs->col_ids.data(), qs->d_col_ids, qs->nq, qs->d_dense, qs->d_col_partial, qs->d_nent));
    if (qs->d_dense_lut) MK_TRY(launch_dense_lut(c, qs->d_dense, (uint32_t)(qs->dense_q.size() / 4), qs->d_dense_lut));
    MK_TRY(launch_scan_counts(c, qs));
    qs->sketched = true;
    return MK_OK;
}

int qset_sketch_only(mk_ctx *c, mk_qset *qs)
{
    if (qs->columns) return qset_sketch_columns(c, qs);
    MK_TRY(ensure_bloom_summary(c));
    ScopedTimer t(c, 0);
    MK_TRY(launch_query_sketch_short(c, qs));
    if (!qs->long_q.empty()) {
        if (!c->d_long_table) MK_TRY(c->d_long_table.alloc(c->P));
        // neighbours in the set share one run of the build's packed kernels and one gate-and-append launch; shapes those
        // kernels do not take (h > 22) go one by one through the atomic kernel
        MK_TRY(ensure_build_scratch(c, 0, 0, false));
        // long reads and contigs (up to 2^18 k-mers): per-query hash tables, O(length) -- no 2^h table is touched
        std::vector<uint32_t> mid, rest;
        for (uint32_t q : qs->long_q) {
            const uint64_t len = qs->h_off[q + 1] - qs->h_off[q];
            (query_is_mid_length(c, len - c->p.k) ? mid : rest).push_back(q);
        }
        // (MIEKKI_MID_SLOTS: fewer slots per round than the scratch holds -- the tests make small sets take several rounds)
        static const uint64_t slot_cap = [] { const char *e = getenv("MIEKKI_MID_SLOTS"); return e ? (uint64_t)std::max(1L, atol(e)) : ~0ull; }();
        MK_TRY(launch_query_sketch_mid(c, qs, mid, reinterpret_cast<unsigned long long *>(c->d_tables.p),
                                       std::min<uint64_t>((uint64_t)c->build_batch * c->P, slot_cap)));
        const std::vector<uint32_t> &long_q = rest;
        for (size_t i = 0; i < long_q.size();) {
            uint32_t n = 1;
            while (i + n < long_q.size() && n < c->build_batch && long_q[i + n] == long_q[i] + n) ++n;
            bool done = false;
            MK_TRY(launch_query_sketch_long_batch(c, qs, long_q[i], n, &done));     // (a loner too: a run of one)
            if (!done)
                for (uint32_t j = 0; j < n; ++j) MK_TRY(launch_query_sketch_long(c, qs, long_q[i + j]));
            i += n;
        }
    }
    if (!qs->dense_q.empty()) {
        if (!c->d_long_table) MK_TRY(c->d_long_table.alloc(c->P));
        // the same for whole-genome (dense) queries, up to a build batch at a time
        MK_TRY(ensure_build_scratch(c, 0, 0, false));
        for (uint32_t slot = 0; slot < qs->dense_q.size();) {
            if (qs->dense_q[slot] == 0xffffffffu) { ++slot; continue; }
            uint32_t n = 1;
            while (slot + n < qs->dense_q.size() && n < c->build_batch && qs->dense_q[slot + n] == qs->dense_q[slot] + n) ++n;
            bool done = false;
            MK_TRY(launch_query_sketch_dense_batch(c, qs, slot, n, &done));
            if (!done)
                for (uint32_t j = 0; j < n; ++j) MK_TRY(launch_query_sketch_dense(c, qs, slot + j));
            slot += n;
        }
        // the field tables the dense scan looks bytes up in (scan_dense_lut_kernel)
        if (qs->d_dense_lut) MK_TRY(launch_dense_lut(c, qs->d_dense, (uint32_t)(qs->dense_q.size() / 4), qs->d_dense_lut));
    }
    MK_TRY(launch_scan_counts(c, qs));
    qs->sketched = true;
    return MK_OK;
}

// Sketch, Bloom gate and slab range table of a set are functions of the set and of the index
// (Bloom cells, slab shape): they are kept until either changes (the index generation stamp)
// or the caller asks for a fresh pass (mk_qset_invalidate).
static int qset_sketch(mk_ctx *c, mk_qset *qs)
{
    if (qs->sketched && qs->gen == c->gen) return MK_OK;
    qs->sketched = false;
    MK_TRY(qset_sketch_only(c, qs));
    MK_TRY(qset_prepare_slab(c, qs));
    qs->gen = c->gen;
    return MK_OK;
}

static uint32_t ntiles_of(const mk_ctx *c)
{
    return (uint32_t)(((uint64_t)c->G * c->W + kTileBytes - 1) / kTileBytes);
}

// Ranges of the slab schedule: the (2^h / S) x 1 KiB column slab the waves in flight
// share should fit the 256 MiB Infinity Cache with room to spare (target 128 MiB).
static uint32_t slab_ranges(const mk_ctx *c)
{
    uint64_t target = 128ull << 20;
    if (const char *e = getenv("MIEKKI_SLAB_MIB")) {             // tuning knob
        const long v = atol(e);
        if (v >= 1 && v <= 4096) target = (uint64_t)v << 20;
    }
    const uint64_t slab = (uint64_t)c->P * kTileBytes;
    uint32_t S = 1;
    while (S < 32 && slab / S > target) S <<= 1;
    return S;
}

// The query groups' merged lists of a set with a range table (scan_kernel.hpp: scan_group_kernel): groups of kGroupQ
// queries (MIEKKI_SCAN_GROUPS=0: none, one query per wave, scan_slab_kernel), each list ordered by windows of
// 2^MIEKKI_GROUP_WINDOW partitions (1,024: 1 MiB of one tile's row pieces, a quarter of an XCD's L2).  *made: the set has them.
static int qset_group_lists(mk_ctx *c, mk_qset *qs, bool *made)
{
    uint32_t wshift = 10;
    if (const char *e = getenv("MIEKKI_GROUP_WINDOW")) { const long v = atol(e); if (v >= 4 && v <= 24) wshift = (uint32_t)v; }
    *made = false;
    if (const char *e = getenv("MIEKKI_SCAN_GROUPS")) if (atol(e) == 0) return MK_OK;
    const uint32_t rows_per_range = c->P / qs->S;
    if (rows_per_range == 0) return MK_OK;
    // (the last range may hold up to S - 1 rows more: they fall into its last window)
    while (((rows_per_range - 1) >> wshift) + 1 > kGroupCells / kGroupQ) ++wshift;
    const uint32_t nwin = ((rows_per_range - 1) >> wshift) + 1;
    if (!qs->d_glist) MK_TRY(dev_alloc(&qs->d_glist, std::max<uint64_t>(qs->h_ent_off[qs->nq], 1)));
    MK_TRY(launch_group_lists(c, qs, wshift, nwin));
    *made = true;
    return MK_OK;
}

// The query blocks' lists of a set with a range table (scan_kernel.hpp: scan_block_kernel), for sets of at least
// MIEKKI_SCAN_BLOCK_MIN_QUERIES queries (a block's worth: fewer queries share too few row pieces); MIEKKI_SCAN_BLOCKS=0:
// none (the groups' path), MIEKKI_SCAN_BLOCK_QUERIES: fewer queries per block than the LDS holds (the tests' small sets),
// MIEKKI_SCAN_BLOCK_SUB_FAST: the order of the kernel's work items (1, 2, 4 or 8 sub-tiles fastest; kBlockSubFast).
// *made: the set has them, in blocks of qs->block_q queries, walked in the order qs->block_sub_fast.
static int qset_block_lists(mk_ctx *c, mk_qset *qs, bool *made)
{
    *made = false;
    if (const char *e = getenv("MIEKKI_SCAN_BLOCKS")) if (atol(e) == 0) return MK_OK;
    uint32_t B = kBlockQ, min_q = kBlockQ;
    if (const char *e = getenv("MIEKKI_SCAN_BLOCK_QUERIES")) { const long v = atol(e); if (v >= 1 && v < (long)kBlockQ) B = (uint32_t)v; }
    if (const char *e = getenv("MIEKKI_SCAN_BLOCK_MIN_QUERIES")) min_q = (uint32_t)std::max(1L, atol(e));
    // (taken as it stands: launch_scan_slab refuses what is not 1, 2, 4 or 8 -- the query fails with its error, nothing is launched)
    qs->block_sub_fast = kBlockSubFast;
    if (const char *e = getenv("MIEKKI_SCAN_BLOCK_SUB_FAST")) qs->block_sub_fast = (uint32_t)std::max(0L, std::min(atol(e), 0x7fffffffL));
    // (a packet names its partition by 24 bits from its range's first)
    if (qs->nq < min_q || c->P / qs->S == 0 || (uint64_t)c->P / qs->S + qs->S > (1u << 24)) return MK_OK;
    const uint64_t nblk = (qs->nq + B - 1) / B;
    // (a packet per entry at most, and every (block, range) list's padding to a whole step: block_list_kernel)
    MK_TRY(dev_grow(qs->d_bpackets, qs->bpackets_cap, std::max<uint64_t>(qs->h_ent_off[qs->nq], 1) + nblk * qs->S * kBlockStepPackets));
    MK_TRY(dev_grow(qs->d_binfo, qs->binfo_cap, nblk * qs->S));
    qs->block_q = B;
    MK_TRY(launch_block_lists(c, qs));
    *made = true;
    return MK_OK;
}

// Prepare the slab schedule for a sketched set: range boundaries per query, and the
// check that every (query, range) fits the packed 8/16-bit counters.  Sets with long
// (unsorted) queries, or that fail the check, use the plain schedule.  The one place that says which kernel walks
// the ranges (qs->ranged); the knobs are read here, at every preparation.
static int qset_prepare_slab(mk_ctx *c, mk_qset *qs)
{
    uint32_t S = slab_ranges(c);
    qs->slab_ok = false;
    qs->ranged = RangedScan::PerWave;
    qs->chunk = 0;
    if (!qs->long_q.empty() || !qs->dense_q.empty() || !qs->nq) { qs->S = S; return MK_OK; }
    const uint32_t limit = c->W == 1 ? 255u : 65535u;
    // A handful of queries has no reuse to schedule -- what it needs is parallelism: one wave per
    // (query, tile) would walk ~900 entries in ~110 dependent steps (a single query: 13 waves on
    // 256 CUs).  So small sets cut every entry list into S pieces BY COUNT: S x as many waves, each
    // a few steps long, no range table, and no eligibility check (a piece holds at most `chunk`
    // <= 255 entries by construction), i.e. no host round trip either.
    uint32_t small_below = 512;
    if (const char *e = getenv("MIEKKI_SLAB_MIN_QUERIES")) small_below = (uint32_t)std::max(0L, atol(e));   // tests force the range-table path
    // (with cold rows the ranges are cut by partition whatever the set's size: whole cold ranges are then staged
    // through HBM once per chunk, where pieces cut by count would have every wave read its rows over PCIe)
    if (qs->nq < small_below && !has_cold(c)) {
        const uint64_t waves = (uint64_t)ntiles_of(c) * qs->nq;
        // (up to eight pieces: that is what select_kernel sums with its words prefetched; more only
        // when the packed counters ask for it)
        uint32_t Sc = (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(1, (4096 + waves - 1) / std::max<uint64_t>(waves, 1)));
        Sc = std::max<uint32_t>(Sc, (qs->short_max_nk + limit - 1) / limit);
        Sc = std::max<uint32_t>(Sc, 1);
        qs->S = Sc;
        qs->chunk = std::max<uint32_t>(1, (qs->short_max_nk + Sc - 1) / Sc);
        qs->ranged = RangedScan::ByCount;
        qs->slab_ok = true;
        return MK_OK;
    }
    if (S < 2) { qs->S = S; return MK_OK; }
    // longer queries need more (smaller) ranges to keep every (query, range) within the
    // packed counters: aim at <= 180 entries per range on average, the device check
    // below still decides
    while (S < 64 && (uint64_t)qs->short_max_nk > (uint64_t)S * (limit * 7 / 10)) S <<= 1;
    if (qs->S != S || !qs->d_split) {
        if (!(qs->split_in_arena && S <= qs->split_room)) {        // more ranges than the set reserved room for
            if (!qs->split_in_arena) dev_free(qs->d_split);
            qs->split_in_arena = false; qs->d_split = nullptr;
            MK_TRY(dev_alloc(&qs->d_split, (uint64_t)qs->nq * (S + 1)));
        }
        qs->S = S;
    }
    if (!c->d_flag) MK_TRY(c->d_flag.alloc(1));
    MK_HIP(hipMemsetAsync(c->d_flag, 0, 4, c->stream));
    MK_TRY(launch_query_split(c, qs, S, limit, c->d_flag));
    uint32_t flag = 1;
    MK_HIP(hipMemcpyAsync(&flag, c->d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    qs->slab_ok = flag == 0;
    if (qs->slab_ok) {
        bool made;
        MK_TRY(qset_block_lists(c, qs, &made));
        if (made) qs->ranged = RangedScan::Blocks;
        else {
            MK_TRY(qset_group_lists(c, qs, &made));
            if (made) qs->ranged = RangedScan::Groups;
        }
    }
    return MK_OK;
}

static uint32_t tile_genomes(const mk_ctx *c) { return kTileBytes / c->W; }
// entries of one query's scores in the tile-major matrix (whole tiles)
static uint64_t score_row_entries(const mk_ctx *c) { return (uint64_t)ntiles_of(c) * tile_genomes(c); }

// queries per chunk so that the chunk's score matrix stays within ~4 GiB
// Bytes a query chunk's score / partial buffer may take: `want`, but never more than what is
// already allocated or a third of the free device memory (a nearly full GPU scans in smaller
// chunks instead of failing).
static uint64_t chunk_budget(uint64_t want, uint64_t have)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return want;
    // (what an ingest of gzip'd genomes left with the inflater counts as free: given back when the chunk would shrink for it)
    if (free_b / 3 < want && want > have && gz_release_idle_blocks() && hipMemGetInfo(&free_b, &total_b) != hipSuccess) return want;
    return std::max<uint64_t>(std::min<uint64_t>(want, std::max<uint64_t>(have, free_b / 3)), 64ull << 20);
}

static uint32_t chunk_queries(const mk_ctx *c, uint32_t nq)
{
    const uint64_t budget = chunk_budget(4ull << 30, c->d_scores.cap * 4) / 4;
    const uint64_t per = std::max<uint64_t>(1, budget / std::max<uint64_t>(score_row_entries(c), 1));
    return (uint32_t)std::min<uint64_t>(per, std::max<uint32_t>(nq, 1));
}

static int ensure_scores(mk_ctx *c, uint64_t rows) { return c->d_scores.grow(rows * score_row_entries(c)); }

// two staging buffers in HBM for cold rows (the copy of one piece runs beside the scan of the previous one), each
// `unit` rows or a multiple of it: as many as fit a sixteenth of the hot part, at least `unit`, at most the cold rows
static int ensure_cold_stage(mk_ctx *c, uint64_t unit)
{
    unit = std::max<uint64_t>(unit, 1);
    if (c->d_cold_stage && c->cold_stage_rows >= unit && c->cold_stage_rows % unit == 0) return MK_OK;
    MK_HIP(hipStreamSynchronize(c->stream));
    MK_HIP(hipStreamSynchronize(c->copy_stream));
    c->cold_stage_rows = 0;
    uint64_t rows = std::max<uint64_t>(unit, (uint64_t)c->P_hot / 16 / unit * unit);
    rows = std::min<uint64_t>(rows, ((uint64_t)c->P - c->P_hot + unit - 1) / unit * unit + unit);
    MK_TRY(c->d_cold_stage.alloc(2 * rows * c->ld));
    c->cold_stage_rows = rows;
    for (mk::Event &e : c->ev_cold) MK_TRY(e.create());
    return MK_OK;
}

// Row windows of a matrix with cold rows: rows [0, first_row) (first_row <= P_hot) in one launch, in HBM where they lie;
// then the rest, a staging buffer's worth at a time (a multiple of `unit` rows) -- copied on the copy stream beside the
// launch over the previous window (rows below P_hot by a device copy, the cold ones from host memory) and presented to
// the kernel as "the matrix" by a shifted base.  launch(M, Mc, P_hot, row_lo, row_hi, first).
template <typename Launch>
static int scan_windows(mk_ctx *c, uint64_t first_row, uint64_t unit, Launch launch)
{
    MK_TRY(ensure_cold_stage(c, unit));
    MK_TRY(ensure_zstage(c, c->cold_stage_rows));
    hipEvent_t ev_enter = c->ev_cold[4];
    const mk::Event *ev_copy = c->ev_cold, *ev_scan = c->ev_cold + 2;
    // the copies may start as soon as everything queued so far (earlier launches out of the stage) is done
    MK_HIP(hipEventRecord(ev_enter, c->stream));
    MK_HIP(hipStreamWaitEvent(c->copy_stream, ev_enter, 0));
    bool first = true;
    if (first_row) {                                                // ... i.e. beside the launch over the rows in HBM
        const MatRef m = mat_ref(c);
        MK_TRY(launch((const uint8_t *)m.hot, (const uint8_t *)m.cold_m, m.P_hot, 0u, (uint32_t)first_row, true));
        first = false;
    }
    uint32_t i = 0;
    for (uint64_t r = first_row; r < c->P; r += c->cold_stage_rows, ++i) {
        const uint64_t last = std::min<uint64_t>(r + c->cold_stage_rows, c->P);          // rows [r, last)
        const uint64_t hot_rows = r < c->P_hot ? std::min<uint64_t>(last, c->P_hot) - r : 0;
        const int b = (int)(i & 1u);
        uint8_t *stage = c->d_cold_stage + (uint64_t)b * c->cold_stage_rows * c->ld;
        if (i >= 2) MK_HIP(hipStreamWaitEvent(c->copy_stream, ev_scan[b], 0));     // the launch that read this buffer last
        if (hot_rows) MK_HIP(hipMemcpyAsync(stage, c->d_M + r * c->ld, hot_rows * c->ld, hipMemcpyDeviceToDevice, c->copy_stream));
        // (packed rows: their packed bytes cross PCIe, cold.hip)
        if (r + hot_rows < last) MK_TRY(stage_cold_rows(c, r + hot_rows, last, stage + hot_rows * c->ld, b, c->copy_stream));
        MK_HIP(hipEventRecord(ev_copy[b], c->copy_stream));
        MK_HIP(hipStreamWaitEvent(c->stream, ev_copy[b], 0));
        // row p of the window now lives at stage + (p - r) * ld
        MK_TRY(launch(stage - r * c->ld, (const uint8_t *)nullptr, c->P, (uint32_t)r, (uint32_t)last, first));
        first = false;
        MK_HIP(hipEventRecord(ev_scan[b], c->stream));
    }
    return MK_OK;
}

// scan queries [q0, q1) of the set into d_scores laid out as `lay` describes (the
// tile-major layout is per call: its tile stride is (q1 - q0) * genomes per tile)
static int qset_scan(mk_ctx *c, mk_qset *qs, uint32_t q0, uint32_t q1, uint32_t *d_scores, const ScoreLayout &lay)
{
    if (q1 <= q0 || c->G == 0) return MK_OK;
    const uint32_t nt = ntiles_of(c);
    const uint32_t per_launch = std::max<uint32_t>(1, 0x7ffffff0u / nt);
    const bool windowed = has_cold(c);                             // cold rows: one launch per window of rows
    // One pass over the row windows for both kernels (a cold window is copied to HBM once): the sparse kernel
    // first -- in the first window it also writes the zero rows of the dense queries (scan_n = 0) -- then the dense
    // kernel, which adds the whole-genome queries' scores, up to eight queries per pass over the rows.
    auto launch = [&](const uint8_t *M, const uint8_t *Mc, uint32_t P_hot, uint32_t row_lo, uint32_t row_hi, bool first) {
        for (uint32_t q = q0; q < q1; q += per_launch) {
            const uint32_t n = std::min(per_launch, q1 - q);
            ScanArgs a;
            a.M = M; a.Mc = Mc; a.P_hot = P_hot; a.ld = c->ld; a.G = c->G; a.ntiles = nt; a.nq = n; a.q_begin = q;
            a.entries = qs->d_entries; a.ent_off = qs->d_ent_off; a.nent = qs->d_scan_n;
            a.scores = d_scores + (uint64_t)(q - q0) * lay.q_stride;
            a.score_tile_stride = lay.tile_stride; a.score_q_stride = lay.q_stride; a.score_vec = lay.vec;
            a.windowed = windowed ? 1u : 0u; a.row_lo = row_lo; a.row_hi = row_hi; a.accumulate = first ? 0u : 1u;
            ScopedTimer t(c, 1);
            MK_TRY(launch_scan(c, a));
        }
        if (qs->dense_q.empty()) return (int)MK_OK;
        DenseArgs d;
        d.M = M; d.Mc = Mc; d.P_hot = P_hot; d.ld = c->ld; d.G = c->G; d.ntiles = nt; d.P = c->P;
        d.row_lo = row_lo; d.row_hi = row_hi;
        d.ngroups = (uint32_t)(qs->dense_q.size() / 4);
        d.rows_per_item = std::min<uint32_t>(row_hi - row_lo, dense_chunk_rows((d.ngroups + 1) / 2));   // (the table kernel counts in 14 or 13 bit planes)
        d.nchunks = (row_hi - row_lo + d.rows_per_item - 1) / d.rows_per_item;
        d.dense = qs->d_dense; d.dense_q = qs->d_dense_q; d.q0 = q0; d.q1 = q1; d.scores = d_scores;
        d.lut = qs->d_dense_lut; d.noctets = (d.ngroups + 1) / 2;
        d.score_tile_stride = lay.tile_stride; d.score_q_stride = lay.q_stride; d.empty = c->empty;
        ScopedTimer t(c, 1);
        return launch_scan_dense(c, d);
    };
    if (!windowed) return launch(c->d_M, (const uint8_t *)nullptr, c->P, 0u, c->P, true);
    return scan_windows(c, c->P_hot, std::max<uint64_t>(1, c->P / 64), launch);
}

// ---- slab schedule: per-range partial counts instead of a u32 score matrix
static uint64_t partial_bytes_per_query(const mk_ctx *c, uint32_t S) { return (uint64_t)ntiles_of(c) * S * kTileBytes; }

static uint32_t chunk_queries_slab(const mk_ctx *c, uint32_t nq, uint32_t S)
{
    const uint64_t budget = chunk_budget(16ull << 30, c->d_partials.cap);
    uint64_t per = std::max<uint64_t>(1, budget / std::max<uint64_t>(partial_bytes_per_query(c, S), 1));
    per = std::min<uint64_t>(per, 0x7ffffff0ull / std::max<uint64_t>((uint64_t)ntiles_of(c) * S, 1));   // one launch
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(per, 1), std::max<uint32_t>(nq, 1));
}

static int qset_scan_slab(mk_ctx *c, mk_qset *qs, uint32_t q0, uint32_t q1)
{
    const uint32_t rows_per_range = qs->S ? c->P / qs->S : c->P;
    // everything in HBM -- or ranges cut by count (small sets), which do not map to partition ranges, or no ranges at
    // all: cold rows, if any, are then read in place over PCIe -- as they are, so unpack them BEFORE the matrix's
    // addresses are taken (need_raw_cold gives the cold rows a new home)
    const bool in_place = !has_cold(c) || qs->ranged == RangedScan::ByCount || qs->S < 2 || rows_per_range == 0;
    if (has_cold(c) && in_place) MK_TRY(need_raw_cold(c));
    SlabArgs a;
    a.M = c->d_M; a.Mc = mat_ref(c).cold_m; a.P_hot = c->P_hot; a.ld = c->ld; a.G = c->G; a.ntiles = ntiles_of(c);
    a.nq = q1 - q0; a.q_begin = q0; a.S = qs->S; a.r_begin = 0; a.r_count = qs->S;
    a.entries = qs->d_entries; a.ent_off = qs->d_ent_off; a.split = qs->d_split; a.partials = c->d_partials;
    a.kind = qs->ranged;
    switch (a.kind) {                                              // what that kernel reads besides
    case RangedScan::ByCount: a.chunk = qs->chunk; a.nent = qs->d_scan_n; break;
    case RangedScan::PerWave: break;
    case RangedScan::Groups: a.lists = qs->d_glist; a.nset = qs->nq; break;
    case RangedScan::Blocks: a.bpackets = qs->d_bpackets; a.binfo = qs->d_binfo; a.block_q = qs->block_q; a.block_sub_fast = qs->block_sub_fast; a.range_rows = rows_per_range; break;
    }
    c->stats.scan_slab_launches++;
    if (in_place) {
        ScopedTimer t(c, 1);
        return launch_scan_slab(c, a);
    }
    // Cold partition ranges are STREAMED: a range's rows are copied once into a staging buffer in HBM and every query
    // of the chunk scans them there, instead of each wave fetching its 1 KiB pieces over PCIe.  The range the hot /
    // cold boundary falls into is staged as a whole.
    const uint64_t hot_rows = (uint64_t)(c->P_hot / rows_per_range) * rows_per_range;     // of the ranges that lie in HBM completely
    return scan_windows(c, hot_rows, rows_per_range, [&](const uint8_t *M, const uint8_t *Mc, uint32_t P_hot, uint32_t row_lo, uint32_t row_hi, bool) {
        a.M = M; a.Mc = Mc; a.P_hot = P_hot;
        a.r_begin = row_lo / rows_per_range; a.r_count = (row_hi - row_lo) / rows_per_range;
        ScopedTimer t(c, 1);
        return launch_scan_slab(c, a);
    });
}

// genome_size / sketch_size per genome as floats, current as of the index generation
static int ensure_ratio(mk_ctx *c)
{
    if (c->d_ratio.cap < c->capG) c->ratio_gen = 0;
    MK_TRY(c->d_ratio.grow(c->capG));
    if (c->ratio_gen != c->gen) { MK_TRY(launch_ratio(c, c->d_ratio, c->capG)); c->ratio_gen = c->gen; }
    return MK_OK;
}

// queries per chunk of a sketched set's scan, in the set's schedule
static uint32_t qset_chunk(const mk_ctx *c, const mk_qset *qs)
{
    return qs->slab_ok ? chunk_queries_slab(c, qs->nq, qs->S) : chunk_queries(c, qs->nq);
}

// the buffer of a chunk of `per` queries -- their partials (slab schedule) or score rows (plain) -- and `replay` more
// row-major score rows for replays: at d_scores (slab), or behind the chunk's rows
static int ensure_chunk(mk_ctx *c, const mk_qset *qs, uint32_t per, uint32_t replay)
{
    if (!qs->slab_ok) return ensure_scores(c, (uint64_t)per + replay);
    MK_TRY(c->d_partials.grow((uint64_t)per * partial_bytes_per_query(c, qs->S)));
    return replay ? ensure_scores(c, replay) : MK_OK;
}

// THE schedule choice: scan queries [q0, q1) of a sketched set into the chunk buffer -- the slab schedule's partials, or
// tile-major scores
static int qset_scan_chunk(mk_ctx *c, mk_qset *qs, uint32_t q0, uint32_t q1)
{
    if (qs->slab_ok) return qset_scan_slab(c, qs, q0, q1);
    return qset_scan(c, qs, q0, q1, c->d_scores, score_layout_tiles(c->W, q1 - q0));
}

// what qset_scan_chunk left of queries [q0, q0 + n), for the kernels that read it against the two thresholds
static int chunk_view(mk_ctx *c, const mk_qset *qs, uint32_t q0, uint32_t n, uint32_t min_score, double min_inter, ChunkView *v)
{
    const bool slab = qs->slab_ok;
    v->scores = slab ? nullptr : c->d_scores; v->partials = slab ? c->d_partials : nullptr;
    v->nent = slab ? qs->d_nent + q0 : nullptr; v->S = qs->S; v->W = c->W;
    v->tile_genomes = tile_genomes(c); v->G = c->G; v->nq = n;
    v->min_score = min_score; v->min_inter = min_inter; v->sketch_size = c->d_sketch_size; v->genome_size = c->d_genome_size;
    v->genome_id_base = c->p.genome_id_base; v->ratio = nullptr;
    if (slab) {                                                    // the slab schedule's kernels screen with one float per genome
        MK_TRY(ensure_ratio(c));
        v->ratio = c->d_ratio;
    }
    return MK_OK;
}

// The one pass over a sketched set, chunk by chunk in the set's schedule: each chunk is scanned ONCE and handed to
// body(q0, q1, view).  replay_rows: row-major score rows kept beside the chunk for replays (*d_replay, when asked for, is
// where); min_chunks: cut the set into at least that many chunks (query blocks: into chunks of no fewer than kBlockShareBlocks
// blocks, so possibly fewer chunks).  MIEKKI_CHUNK_QUERIES caps a chunk's queries: the tests
// make small sets take several chunks.
template <typename Body>
static int for_chunks(mk_ctx *c, mk_qset *qs, uint32_t replay_rows, uint32_t min_chunks, uint32_t min_score, double min_inter, Body body,
                      uint32_t **d_replay = nullptr)
{
    uint32_t per = qset_chunk(c, qs);
    if (min_chunks > 1) {
        uint32_t cut = std::max<uint32_t>(1, (qs->nq + min_chunks - 1) / min_chunks);
        // (query blocks share row pieces among the blocks of ONE launch: a launch of three or four blocks scans 29 % slower per
        // query than one of sixteen, more than an exchange hidden behind the next chunk gives back -- profiles/r13_scan_block_order.txt, f)
        if (qs->slab_ok && qs->ranged == RangedScan::Blocks) cut = std::max(cut, kBlockShareBlocks * qs->block_q);
        per = std::min(per, cut);
    }
    // (query blocks: a chunk of whole blocks, where it holds one at all -- a block cut by a chunk boundary is counted on both sides)
    if (qs->slab_ok && qs->ranged == RangedScan::Blocks && per > qs->block_q) per -= per % qs->block_q;
    if (const char *e = getenv("MIEKKI_CHUNK_QUERIES")) { const long v = atol(e); if (v >= 1) per = (uint32_t)std::min<long>(per, v); }
    MK_TRY(ensure_chunk(c, qs, per, replay_rows));
    if (d_replay) *d_replay = c->d_scores + (qs->slab_ok ? 0 : (uint64_t)per * score_row_entries(c));
    for (uint32_t q0 = 0; q0 < qs->nq; q0 += per) {
        const uint32_t q1 = std::min(qs->nq, q0 + per);
        MK_TRY(qset_scan_chunk(c, qs, q0, q1));
        ChunkView v;
        MK_TRY(chunk_view(c, qs, q0, q1 - q0, min_score, min_inter, &v));
        MK_TRY(body(q0, q1, v));
    }
    return MK_OK;
}

// entrants of filter_results' heap for the queries of a scanned chunk (see select.hip): (d_count, d_cand) or d_rows
static int qset_select(mk_ctx *c, const ChunkView &v, uint32_t nresults, uint32_t cap, uint32_t *d_count, mk_hit *d_cand, uint64_t *d_rows)
{
    const SelectArgs a{v, nresults, cap, d_count, d_cand, d_rows};
    ScopedTimer t(c, 2);
    return launch_select(c, a);
}

// the list walk's arguments (list.hip, family.hip) for queries [q_lo, q_lo + q_n) of a scanned chunk
static ListArgs list_args(const ChunkView &v, uint32_t q_lo, uint32_t q_n, uint32_t *count, const uint64_t *rec_off, uint64_t *rec)
{
    return ListArgs{v.scores, v.partials, v.nent, v.S, v.W, v.tile_genomes, v.G, v.nq, q_lo, q_n, v.min_score, v.min_inter,
                    v.sketch_size, v.genome_size, v.genome_id_base, v.ratio, count, rec_off, rec};
}

// The reference's loop over ONE query's dense score row (Miekki.cpp:381-384), for what the device does not order -- rows that
// overflowed, top-N sizes beyond the device selection, NaN intersections: query q is scanned into d_row (one row-major
// score row), the row comes to the host, and the genomes that pass both thresholds are left in `full` in ascending id.
static int replay_query(mk_ctx *c, mk_qset *qs, uint32_t q, uint32_t *d_row, uint32_t min_score, double min_inter, std::vector<mk_hit> &full)
{
    std::vector<uint32_t> row(c->G);
    MK_TRY(qset_scan(c, qs, q, q + 1, d_row, score_layout_rows(c->W, score_row_entries(c), c->G)));
    MK_HIP(hipMemcpyAsync(row.data(), d_row, (size_t)c->G * 4, hipMemcpyDeviceToHost, c->stream));
    MK_HIP(hipStreamSynchronize(c->stream));
    full.clear();
    for (uint32_t g = 0; g < c->G; ++g) {
        if (row[g] < min_score) continue;
        const double jac = (double)row[g] / c->h_sketch_size[g];
        const double inter = jac * c->h_genome_size[g];
        if (inter < min_inter) continue;
        full.push_back(mk_hit{g + c->p.genome_id_base, row[g], jac, inter});
    }
    return MK_OK;
}

// what a call's scans compared, from its queries' active partition counts
static void add_scan_stats(mk_ctx *c, const std::vector<uint32_t> &act)
{
    uint64_t a = 0;
    for (uint32_t v : act) a += v;
    c->stats.active_partitions += a;
    c->stats.comparisons += a * c->G;
    c->stats.scan_algo_bytes += a * c->G * c->W + 4ull * act.size() * c->G;
}

// ---- what the sinks of api_sinks.hip stand on (declared in mk_internal.hpp) ----------------------------------------------
int refuse_nan_lists(mk_ctx *c, uint32_t min_score)
{
    if (!nan_candidates_possible(c, min_score)) return MK_OK;
    set_error("min_score 0 over an index with empty sketches yields NaN intersections: whether such a genome is listed follows no order");
    return MK_ERR_UNSUPPORTED;
}

// fn(leaf, places) for every leaf of a set that has something to scan, sketched: the set itself (places = null), or the two
// parts of a mixed set, each with its own schedule and its queries' places in the set
int qset_leaves(mk_ctx *c, mk_qset *qs, const std::function<int(mk_qset *, const std::vector<uint32_t> *)> &fn)
{
    for (int i = 0; i < (qs->part[0] ? 2 : 1); ++i) {
        mk_qset *leaf = qs->part[0] ? qs->part[i] : qs;
        if (leaf->from_index && leaf->nq) MK_TRY(qset_sketch(c, leaf));   // (an emptied index: the set's genomes are gone, MK_ERR_STATE)
        if (!leaf->nq || !c->G) continue;
        MK_TRY(qset_sketch(c, leaf));
        MK_TRY(fn(leaf, qs->part[0] ? &qs->part_q[i] : nullptr));
    }
    return MK_OK;
}

// THE walk pass over a leaf: every chunk is scanned once and handed whole to sink(q0, args) -- the place in the leaf of the
// chunk's first query, the list walk's arguments for all its queries -- which queues its launch; nothing is waited for
int qset_walk(mk_ctx *c, mk_qset *leaf, uint32_t min_score, double min_inter, const std::function<int(uint32_t, const ListArgs &)> &sink)
{
    return for_chunks(c, leaf, 0, 1, min_score, min_inter, [&](uint32_t q0, uint32_t q1, const ChunkView &v) -> int {
        const ListArgs a = list_args(v, 0, q1 - q0, nullptr, nullptr, nullptr);
        ScopedTimer t(c, 2);
        return sink(q0, a);
    });
}

// A caller's sequences in slices, as mk_query answers very large calls (the device-side set grows with the queries, no result
// depends on the slicing): fn(qs, q0, n) for the uploaded set of sequences [q0, q0 + n), a shell over two parts when mixed
int for_uploaded_slices(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, const std::function<int(mk_qset *, uint32_t, uint32_t)> &fn)
{
    constexpr uint32_t kMaxCall = 1u << 18;
    for (uint32_t q0 = 0; q0 < nq; q0 += kMaxCall) {
        const uint32_t n = std::min(kMaxCall, nq - q0);
        mk_qset *qs = nullptr;
        MK_TRY(mk_qset_upload(c, seqs + q0, lens + q0, n, &qs));
        std::unique_ptr<mk_qset, void (*)(mk_qset *)> guard(qs, qset_release);
        const int rc = fn(qs, q0, n);
        MK_HIP(hipStreamSynchronize(c->stream));                                // before the set's memory goes
        MK_TRY(rc);
    }
    return MK_OK;
}

// ids per set of a pass of the index over itself: whole runs of 64 ids, as many as 2 GiB of query vectors and tables hold (3
// bytes per partition and byte).  MIEKKI_REP_SET_IDS: the tests make small indexes take several sets, whole runs of 64 or not
uint32_t index_set_ids(const mk_ctx *c)
{
    const uint64_t fit = (2ull << 30) / (3ull * c->P * c->W);
    uint32_t per = (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(4096, fit) / 64 * 64);
    if (const char *e = getenv("MIEKKI_REP_SET_IDS")) { const long v = atol(e); if (v >= 1) per = (uint32_t)std::min<long>(per, v); }
    return per;
}

// fn(qs, ids, g0, n) for the index's genomes in sets of `per`: the set of local genomes [g0, g0 + n), ids[] = their reported ids
int for_index_sets(mk_ctx *c, uint32_t per, const std::function<int(mk_qset *, const uint32_t *, uint32_t, uint32_t)> &fn)
{
    std::vector<uint32_t> ids;
    for (uint32_t g0 = 0; g0 < c->G; g0 += per) {
        const uint32_t n = std::min(per, c->G - g0);
        ids.resize(n);
        for (uint32_t j = 0; j < n; ++j) ids[j] = c->p.genome_id_base + g0 + j;
        mk_qset *qs = nullptr;
        MK_TRY(mk_qset_from_index(c, ids.data(), n, &qs));
        const int rc = fn(qs, ids.data(), g0, n);
        mk_qset_free(c, qs);                                       // (waits for the pass)
        MK_TRY(rc);
    }
    return MK_OK;
}

}  // namespace mk

using namespace mk;


// The one split of a mixed set: its short queries (part 0, at most kShortMax k-mers: the slab schedule) and the others
// (part 1: the plain / dense kernels), each in the set's order.  False when the set is not mixed.
struct SetPart {
    std::vector<uint32_t> idx;     // places in the set
    std::vector<const char *> seqs;
    std::vector<uint64_t> lens;
};
static bool split_mixed(const mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, SetPart part[2])
{
    for (uint32_t q = 0; q < nq; ++q) {
        SetPart &p = part[beyond_short_len(c->p.k, lens[q]) ? 1 : 0];
        p.idx.push_back(q); p.seqs.push_back(seqs[q]); p.lens.push_back(lens[q]);
    }
    return !part[0].idx.empty() && !part[1].idx.empty();
}

// transient: the set lives for one mk_query call -- borrowed arena, and no wait for the copy
// (the caller's buffers have been copied into the pinned image; the call's own final wait covers it)
// cuts: the set is one of read pairs -- seqs[q] holds both mates back to back, cuts[q] is mate 1's length (qset_alloc)
// quals: the set carries base qualities -- quals[q] holds lens[q] bytes, in seqs[q]'s order; min_qual is kept with them
static int qset_upload(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, mk_qset **out, bool transient,
                       const uint32_t *cuts = nullptr, const char *const *quals = nullptr, uint32_t min_qual = 0)
{
    mk_qset *qs = nullptr;
    MK_TRY(qset_alloc(c, lens, nq, &qs, transient, cuts, quals != nullptr));
    std::unique_ptr<mk_qset, void (*)(mk_qset *)> guard(qs, qset_release);
    if (cuts && nq) MK_HIP(hipMemcpy(qs->d_cut, cuts, (size_t)nq * 4, hipMemcpyHostToDevice));
    if (quals) {
        qs->min_qual = min_qual;
        std::vector<char> host(qs->total_len + 1);                 // one copy of all the qualities, in d_seq's layout
        for (uint32_t q = 0; q < nq; ++q)
            if (lens[q]) memcpy(host.data() + qs->h_off[q], quals[q], lens[q]);
        if (qs->total_len) MK_HIP(hipMemcpy(qs->d_qual, host.data(), qs->total_len, hipMemcpyHostToDevice));
    }
    constexpr uint64_t kImageMax = 8ull << 20;
    if (qs->head_bytes <= kImageMax) {
        // small batch: ONE copy of a pinned image of (sequences, offsets, entry offsets)
        MK_TRY(ensure_pinned(c->h_stage, qs->head_bytes));
        for (uint32_t q = 0; q < nq; ++q) memcpy(c->h_stage + qs->h_off[q], seqs[q], lens[q]);
        memcpy(c->h_stage + qs->o_off, qs->h_off.data(), ((size_t)nq + 1) * 8);
        memcpy(c->h_stage + qs->o_ent_off, qs->h_ent_off.data(), ((size_t)nq + 1) * 8);
        MK_HIP(hipMemcpyAsync(qs->d_arena, c->h_stage, qs->head_bytes, hipMemcpyHostToDevice, c->stream));
        if (!transient) MK_HIP(hipStreamSynchronize(c->stream));    // the image is reused by the next upload
        *out = guard.release();
        return MK_OK;
    }
    MK_TRY(qset_copy_offsets(c, qs));
    // Short sequences are gathered so that a run of them is ONE copy (100,000 reads must not be
    // 100,000 copies); a long one (a contig, a whole genome) goes straight from the caller's
    // buffer -- a DMA when that buffer is pinned (mk_host_alloc), and no extra pass over it.
    constexpr uint64_t kDirect = 256u << 10;
    std::vector<char> host;
    bool ok = true;
    for (uint32_t q = 0; q < nq && ok;) {
        if (lens[q] >= kDirect) {
            ok = hipMemcpyAsync(qs->d_seq + qs->h_off[q], seqs[q], lens[q], hipMemcpyHostToDevice, c->stream) == hipSuccess;
            ++q;
            continue;
        }
        uint32_t e = q;
        while (e < nq && lens[e] < kDirect && qs->h_off[e + 1] - qs->h_off[q] <= (1ull << 30)) ++e;
        if (e == q) e = q + 1;
        const uint64_t bytes = qs->h_off[e] - qs->h_off[q];
        host.resize(bytes);
        for (uint32_t i = q; i < e; ++i) memcpy(host.data() + (qs->h_off[i] - qs->h_off[q]), seqs[i], lens[i]);
        // synchronous: `host` is reused for the next run
        if (bytes) ok = hipMemcpy(qs->d_seq + qs->h_off[q], host.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
        q = e;
    }
    if (ok) ok = hipStreamSynchronize(c->stream) == hipSuccess;    // the caller's buffers are free again
    if (!ok) { set_error("query upload failed"); return MK_ERR_DEVICE; }
    *out = guard.release();
    return MK_OK;
}

extern "C" {

int mk_qset_upload(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, mk_qset **out)
{
    if (!c || !out || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    // a mixed set: a shell over its two parts (mk_internal.hpp), so that the short ones keep the slab schedule inside
    // ONE mk_qset_run
    SetPart part[2];
    if (!split_mixed(c, seqs, lens, nq, part)) return qset_upload(c, seqs, lens, nq, out, false);
    std::unique_ptr<mk_qset, void (*)(mk_qset *)> shell(new mk_qset(), qset_release);
    mk_qset *qs = shell.get();
    qs->owner = c; qs->nq = nq;
    for (int i = 0; i < 2; ++i) {
        const uint32_t n = (uint32_t)part[i].idx.size();
        MK_TRY(qset_upload(c, part[i].seqs.data(), part[i].lens.data(), n, &qs->part[i], false));
        MK_TRY(dev_alloc(&qs->d_part_q[i], n));
        MK_HIP(hipMemcpy(qs->d_part_q[i], part[i].idx.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        qs->part_q[i] = std::move(part[i].idx);
    }
    *out = shell.release();
    return MK_OK;
}

int mk_qset_upload_pairs(mk_ctx *c, const char *const *seqs1, const uint64_t *lens1, const char *const *seqs2, const uint64_t *lens2,
                         uint32_t nq, mk_qset **out)
{
    if (!c || !out || (nq && (!seqs1 || !lens1 || !seqs2 || !lens2))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    // the two mates of a pair go up back to back, as ONE query of the set; where mate 1 ends is all that tells it from a read
    std::vector<uint64_t> lens(nq), at(nq + 1, 0);
    std::vector<uint32_t> cuts(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        if ((lens1[q] && !seqs1[q]) || (lens2[q] && !seqs2[q])) { set_error("null sequence in pair %u", q); return MK_ERR_ARG; }
        if (pair_kmers(c->p.k, lens1[q], lens2[q]) > kShortMax) {
            set_error("pair %u holds more than %u k-mers (mates of %llu and %llu characters): read pairs are short reads", q, kShortMax,
                      (unsigned long long)lens1[q], (unsigned long long)lens2[q]);
            return MK_ERR_UNSUPPORTED;
        }
        lens[q] = lens1[q] + lens2[q]; cuts[q] = (uint32_t)lens1[q];
        at[q + 1] = at[q] + lens[q];
    }
    std::vector<char> joined(at[nq] + 1);
    std::vector<const char *> seqs(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        seqs[q] = joined.data() + at[q];
        if (lens1[q]) memcpy(joined.data() + at[q], seqs1[q], lens1[q]);
        if (lens2[q]) memcpy(joined.data() + at[q] + lens1[q], seqs2[q], lens2[q]);
    }
    return qset_upload(c, seqs.data(), lens.data(), nq, out, false, cuts.data());
}

int mk_qset_upload_reads(mk_ctx *c, const char *const *seqs1, const uint64_t *lens1, const char *const *quals1,
                         const char *const *seqs2, const uint64_t *lens2, const char *const *quals2, uint32_t nq, uint32_t min_qual,
                         mk_qset **out)
{
    if (!c || !out || (nq && (!seqs1 || !lens1 || !quals1))) { set_error("null argument"); return MK_ERR_ARG; }
    const bool paired = seqs2 || lens2 || quals2;
    if (paired && !(seqs2 && lens2 && quals2)) { set_error("mate 2 needs its sequences, lengths and qualities, all three or none"); return MK_ERR_ARG; }
    if (min_qual > 93) { set_error("min_qual %u: a phred + 33 quality is 0 .. 93", min_qual); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    // a read goes up as it is, a pair's mates back to back (mk_qset_upload_pairs), the qualities beside them; the cuts at the bad
    // bases are found on the device, by every sketch of the set
    std::vector<uint64_t> lens(nq), at(nq + 1, 0);
    std::vector<uint32_t> cuts(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint64_t l2 = paired ? lens2[q] : 0;
        if ((lens1[q] && (!seqs1[q] || !quals1[q])) || (l2 && (!seqs2[q] || !quals2[q]))) {
            set_error("null sequence or quality string in %s %u", paired ? "pair" : "read", q);
            return MK_ERR_ARG;
        }
        if (lens1[q] > kShortMax || l2 > kShortMax || lens1[q] + l2 > kShortMax) {
            set_error("%s %u holds more than %u characters (%llu%s%llu): reads with base qualities are short reads", paired ? "pair" : "read", q,
                      kShortMax, (unsigned long long)lens1[q], paired ? " and " : " + ", (unsigned long long)l2);
            return MK_ERR_UNSUPPORTED;
        }
        lens[q] = lens1[q] + l2; cuts[q] = (uint32_t)lens1[q];
        at[q + 1] = at[q] + lens[q];
    }
    std::vector<char> joined(at[nq] + 1), joined_q(at[nq] + 1);
    std::vector<const char *> seqs(nq), quals(nq);
    for (uint32_t q = 0; q < nq; ++q) {
        seqs[q] = joined.data() + at[q]; quals[q] = joined_q.data() + at[q];
        if (lens1[q]) { memcpy(joined.data() + at[q], seqs1[q], lens1[q]); memcpy(joined_q.data() + at[q], quals1[q], lens1[q]); }
        if (paired && lens2[q]) {
            memcpy(joined.data() + at[q] + lens1[q], seqs2[q], lens2[q]);
            memcpy(joined_q.data() + at[q] + lens1[q], quals2[q], lens2[q]);
        }
    }
    return qset_upload(c, seqs.data(), lens.data(), nq, out, false, paired ? cuts.data() : nullptr, quals.data(), min_qual);
}

int mk_qset_synthetic(mk_ctx *c, uint64_t first_id, uint32_t nq, uint64_t G, uint64_t L, uint64_t qlen,
                      mk_qset **out)
{
    if (!c || !out) { set_error("null argument"); return MK_ERR_ARG; }
    if (!G || qlen == 0 || L <= qlen) { set_error("bad synthetic query shape (need genome_len > query_len)"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    std::vector<uint64_t> lens(nq, qlen);
    mk_qset *qs = nullptr;
    MK_TRY(qset_alloc(c, lens.data(), nq, &qs));
    int rc = qset_copy_offsets(c, qs);
    if (rc == MK_OK) rc = launch_synth_queries(c, first_id, nq, G, L, qlen, qs->d_seq);
    if (rc != MK_OK) { qset_release(qs); return rc; }
    *out = qs;
    return MK_OK;
}

// a set of n whole-genome queries without sequences (colq.hip); its dense vectors are filled by the caller / the sketch step
static int qset_columns(mk_ctx *c, uint32_t n, mk_qset **out)
{
    // (vectors and field tables: 3 P W bytes per query -- the limit the dense path sets itself for uploaded genomes)
    if ((uint64_t)n * c->P * c->W * 3 > (8ull << 30)) { set_error("%u whole-genome queries need more than 8 GiB: ask in smaller sets", n); return MK_ERR_ARG; }
    mk_qset *qs = nullptr;
    MK_TRY(qset_alloc(c, nullptr, n, &qs));
    const int rc = qset_copy_offsets(c, qs);
    if (rc != MK_OK) { qset_release(qs); return rc; }
    *out = qs;
    return MK_OK;
}

int mk_qset_from_index(mk_ctx *c, const uint32_t *ids, uint32_t n, mk_qset **out)
{
    if (!c || !out || !ids) { set_error("null argument"); return MK_ERR_ARG; }
    if (!n) { set_error("no genome ids"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    std::vector<uint32_t> local(n);
    for (uint32_t j = 0; j < n; ++j) {
        if (ids[j] < c->p.genome_id_base || ids[j] - c->p.genome_id_base >= c->G) { set_error("genome id %u is not in this index", ids[j]); return MK_ERR_ARG; }
        local[j] = ids[j] - c->p.genome_id_base;
    }
    mk_qset *qs = nullptr;
    MK_TRY(qset_columns(c, n, &qs));
    qs->from_index = true;
    qs->index_id = c->index_id;
    qs->col_ids = std::move(local);
    if (hipMemcpy(qs->d_col_ids, qs->col_ids.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("genome id upload failed: %s", hipGetErrorString(hipGetLastError()));
        qset_release(qs);
        return MK_ERR_DEVICE;
    }
    *out = qs;
    return MK_OK;
}

int mk_qset_from_columns(mk_ctx *c, const uint8_t *d_cols, uint32_t n, mk_qset **out)
{
    if (!c || !out || !d_cols) { set_error("null argument"); return MK_ERR_ARG; }
    if (!n) { set_error("no columns"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    mk_qset *qs = nullptr;
    MK_TRY(qset_columns(c, n, &qs));
    int rc;
    {
        ScopedTimer t(c, 0);
        rc = launch_dense_from_columns(c, d_cols, n, qs->d_dense, qs->d_col_partial, qs->d_nent);
    }
    if (rc == MK_OK && hipStreamSynchronize(c->stream) != hipSuccess) { set_error("column conversion failed: %s", hipGetErrorString(hipGetLastError())); rc = MK_ERR_DEVICE; }
    if (rc != MK_OK) { qset_release(qs); return rc; }
    *out = qs;                                                       // d_cols is the caller's again
    return MK_OK;
}

int mk_qset_invalidate(mk_ctx *c, mk_qset *qs)
{
    if (!c || !qs) { set_error("null argument"); return MK_ERR_ARG; }
    qs->sketched = false;
    for (int i = 0; i < 2; ++i) if (qs->part[i]) qs->part[i]->sketched = false;
    return MK_OK;
}

void mk_qset_free(mk_ctx *c, mk_qset *qs)
{
    if (c) { (void)hipSetDevice(c->p.device); (void)hipStreamSynchronize(c->stream); }
    qset_release(qs);
}

// mk_qset_run / mk_qset_run_compact: the output is either (d_count, d_cand) or d_rows
// after_chunk (may be null): called once the scan + selection of queries [q0, q1) have been QUEUED on the context's
// stream (comm.hip: the chunk's exchange rows go out on the communicator's stream while the next chunk scans);
// min_chunks: cut the set into at least that many chunks (so that there is a next chunk to overlap with)
}  // extern "C"
namespace mk {
int qset_run(mk_ctx *c, mk_qset *qs, uint32_t nresults, uint32_t min_score, double min_inter, uint32_t cap,
             uint32_t *d_count, mk_hit *d_cand, uint64_t *d_rows, const std::function<int(uint32_t, uint32_t)> *after_chunk,
             uint32_t min_chunks)
{
    if (nresults > kSelectMaxResults) { set_error("device selection supports nresults <= 64"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (nan_candidates_possible(c, min_score)) {
        set_error("min_score 0 over an index with empty sketches yields NaN intersections: use mk_query");
        return MK_ERR_UNSUPPORTED;
    }
    if (qs->part[0]) {
        // a mixed set: each part runs as a set with its own schedule into a buffer of the shell, and a copy kernel puts its
        // rows in their places; the exchange of a sharded run follows the whole set (its blocks are ranges of queries)
        const uint64_t row_bytes = d_rows ? ((uint64_t)cap + 1) * 8 : (uint64_t)cap * sizeof(mk_hit);
        const uint32_t most = (uint32_t)std::max(qs->part_q[0].size(), qs->part_q[1].size());
        const uint64_t need = (uint64_t)most * (row_bytes + 4) + 256;
        MK_TRY(dev_grow(qs->d_part_out, qs->part_out_bytes, need));
        for (int i = 0; i < 2; ++i) {
            mk_qset *p = qs->part[i];
            uint8_t *rows = qs->d_part_out;                            // [n][row_bytes], then (count form) [n] counts
            uint32_t *cnt = reinterpret_cast<uint32_t *>(qs->d_part_out + (((uint64_t)p->nq * row_bytes + 255) & ~255ull));
            MK_TRY(qset_run(c, p, nresults, min_score, min_inter, cap, d_rows ? nullptr : cnt, d_rows ? nullptr : reinterpret_cast<mk_hit *>(rows),
                            d_rows ? reinterpret_cast<uint64_t *>(rows) : nullptr, nullptr, 1));
            MK_TRY(launch_place_rows(c, rows, row_bytes, qs->d_part_q[i], p->nq, d_rows ? reinterpret_cast<uint8_t *>(d_rows) : reinterpret_cast<uint8_t *>(d_cand),
                                     d_rows ? nullptr : cnt, d_count));
        }
        if (after_chunk) MK_TRY((*after_chunk)(0, qs->nq));
        return MK_OK;
    }
    MK_TRY(qset_sketch(c, qs));
    const uint64_t rstride = (uint64_t)cap + 1;
    if (c->G == 0) {                                             // an empty shard still takes part in the exchange
        if (d_rows) MK_HIP(hipMemsetAsync(d_rows, 0, (size_t)qs->nq * rstride * 8, c->stream));
        else MK_HIP(hipMemsetAsync(d_count, 0, (size_t)qs->nq * 4, c->stream));
        if (after_chunk) MK_TRY((*after_chunk)(0, qs->nq));
        return MK_OK;
    }
    return for_chunks(c, qs, 0, min_chunks, min_score, min_inter, [&](uint32_t q0, uint32_t q1, const ChunkView &v) -> int {
        MK_TRY(qset_select(c, v, nresults, cap, d_rows ? nullptr : d_count + q0, d_rows ? nullptr : d_cand + (uint64_t)q0 * cap,
                           d_rows ? d_rows + (uint64_t)q0 * rstride : nullptr));
        return after_chunk ? (*after_chunk)(q0, q1) : (int)MK_OK;
    });
}
}  // namespace mk
extern "C" {

int mk_qset_run(mk_ctx *c, mk_qset *qs, uint32_t nresults, uint32_t min_score, double min_inter, uint32_t cap,
                uint32_t *d_count, mk_hit *d_cand)
{
    if (!c || !qs || !d_count || !d_cand || !cap) { set_error("null argument"); return MK_ERR_ARG; }
    return qset_run(c, qs, nresults, min_score, min_inter, cap, d_count, d_cand, nullptr, nullptr, 1);
}

int mk_qset_run_compact(mk_ctx *c, mk_qset *qs, uint32_t nresults, uint32_t min_score, double min_inter,
                        uint32_t cap, uint64_t *d_rows)
{
    if (!c || !qs || !d_rows || !cap) { set_error("null argument"); return MK_ERR_ARG; }
    return qset_run(c, qs, nresults, min_score, min_inter, cap, nullptr, nullptr, d_rows, nullptr, 1);
}

int mk_qset_scores(mk_ctx *c, mk_qset *qs, uint32_t q0, uint32_t q1, uint32_t *d_scores)
{
    if (!c || !qs || !d_scores) { set_error("null argument"); return MK_ERR_ARG; }
    if (q0 > q1 || q1 > qs->nq) { set_error("query range out of bounds"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (qs->part[0]) {                                           // a mixed set: query by query from the part that holds it
        for (uint32_t q = q0; q < q1; ++q)
            for (int i = 0; i < 2; ++i) {
                const auto it = std::lower_bound(qs->part_q[i].begin(), qs->part_q[i].end(), q);
                if (it == qs->part_q[i].end() || *it != q) continue;
                const uint32_t at = (uint32_t)(it - qs->part_q[i].begin());
                MK_TRY(mk_qset_scores(c, qs->part[i], at, at + 1, d_scores + (uint64_t)(q - q0) * c->G));
            }
        return MK_OK;
    }
    MK_TRY(qset_sketch(c, qs));
    return qset_scan(c, qs, q0, q1, d_scores, score_layout_rows(c->W, c->G, c->G));   // dense rows for the caller
}

int mk_qset_active(mk_ctx *c, mk_qset *qs, uint32_t *active)
{
    if (!c || !qs || !active) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (qs->part[0]) {
        for (int i = 0; i < 2; ++i) {
            std::vector<uint32_t> a(qs->part[i]->nq);
            MK_TRY(mk_qset_active(c, qs->part[i], a.data()));
            for (uint32_t j = 0; j < qs->part[i]->nq; ++j) active[qs->part_q[i][j]] = a[j];
        }
        return MK_OK;
    }
    MK_TRY(qset_sketch(c, qs));
    MK_HIP(hipStreamSynchronize(c->stream));
    if (qs->nq) MK_HIP(hipMemcpy(active, qs->d_nent, (size_t)qs->nq * 4, hipMemcpyDeviceToHost));
    return MK_OK;
}

int mk_query_scores(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t *scores)
{
    if (!c || (nq && (!seqs || !lens || !scores))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!nq || !c->G) return MK_OK;
    mk_qset *qs = nullptr;
    MK_TRY(qset_upload(c, seqs, lens, nq, &qs, true));
    std::unique_ptr<mk_qset, void (*)(mk_qset *)> guard(qs, qset_release);
    MK_TRY(qset_sketch(c, qs));
    const uint32_t per = chunk_queries(c, nq);
    const uint64_t ld = score_row_entries(c);                 // whole tiles per row: 16-byte stores everywhere
    MK_TRY(ensure_scores(c, per));
    for (uint32_t q0 = 0; q0 < nq; q0 += per) {
        const uint32_t q1 = std::min(nq, q0 + per);
        MK_TRY(qset_scan(c, qs, q0, q1, c->d_scores, score_layout_rows(c->W, ld, c->G)));
        MK_HIP(hipMemcpy2DAsync(scores + (uint64_t)q0 * c->G, (size_t)c->G * 4, c->d_scores, (size_t)ld * 4,
                                (size_t)c->G * 4, q1 - q0, hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
    }
    std::vector<uint32_t> act(nq);
    MK_TRY(mk_qset_active(c, qs, act.data()));
    add_scan_stats(c, act);
    return MK_OK;
}


int mk_query(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t nresults,
             uint32_t min_score, double min_inter, mk_hit *hits, uint32_t *nhits, uint32_t *active)
{
    if (!c || (nq && (!seqs || !lens || !hits || !nhits))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    if (!nq) return MK_OK;
    if (!c->G) {
        memset(nhits, 0, (size_t)nq * 4);
        if (active) memset(active, 0, (size_t)nq * 4);     // no column is ever compared
        return MK_OK;
    }
    // Very large calls are answered in slices: the device-side query set (sequences, entry
    // lists) grows with the number of queries, the result does not depend on the slicing.
    constexpr uint32_t kMaxCall = 1u << 18;
    if (nq > kMaxCall) {
        for (uint32_t q0 = 0; q0 < nq; q0 += kMaxCall) {
            const uint32_t n = std::min(kMaxCall, nq - q0);
            MK_TRY(mk_query(c, seqs + q0, lens + q0, n, nresults, min_score, min_inter, hits + (size_t)q0 * nresults,
                            nhits + q0, active ? active + q0 : nullptr));
        }
        return MK_OK;
    }
    // a mixed batch is answered part by part (split_mixed), so that the short queries keep the slab schedule
    SetPart part[2];
    if (nresults > 0 && split_mixed(c, seqs, lens, nq, part)) {
        for (const SetPart &p : part) {
            const uint32_t n = (uint32_t)p.idx.size();
            std::vector<mk_hit> h((size_t)n * nresults);
            std::vector<uint32_t> nh(n), act(n);
            MK_TRY(mk_query(c, p.seqs.data(), p.lens.data(), n, nresults, min_score, min_inter, h.data(), nh.data(), act.data()));
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t q = p.idx[i];
                nhits[q] = nh[i];
                if (active) active[q] = act[i];
                std::copy(h.begin() + (size_t)i * nresults, h.begin() + (size_t)i * nresults + nh[i], hits + (size_t)q * nresults);
            }
        }
        return MK_OK;
    }
    mk_qset *qs = nullptr;
    MK_TRY(qset_upload(c, seqs, lens, nq, &qs, true));
    std::unique_ptr<mk_qset, void (*)(mk_qset *)> guard(qs, qset_release);
    MK_TRY(qset_sketch(c, qs));
    const uint32_t cap = 256;
    const bool on_device = nresults <= kSelectMaxResults && !nan_candidates_possible(c, min_score);
    std::vector<mk_hit> full;
    std::vector<uint32_t> act(nq);
    // a query the device does not answer: replayed over a dense score row of its own
    auto replay = [&](uint32_t q, uint32_t *d_row) -> int {
        MK_TRY(replay_query(c, qs, q, d_row, min_score, min_inter, full));
        nhits[q] = mk_filter_candidates(full.data(), (uint32_t)full.size(), nresults, hits + (size_t)q * nresults);
        return MK_OK;
    };
    if (!on_device) {                                             // every query is a replay
        MK_TRY(ensure_scores(c, 1));
        for (uint32_t q = 0; q < nq; ++q) MK_TRY(replay(q, c->d_scores));
        MK_HIP(hipMemcpy(act.data(), qs->d_nent, (size_t)nq * 4, hipMemcpyDeviceToHost));
    } else {
        // chunks in the set's schedule, and one row-major score row for the replays
        uint32_t *d_replay_row = nullptr;
        MK_TRY(for_chunks(c, qs, 1, 1, min_score, min_inter, [&](uint32_t q0, uint32_t q1, const ChunkView &v) -> int {
            const uint32_t n = q1 - q0;
            MK_TRY(c->d_count.grow(n));
            MK_TRY(c->d_cand.grow((uint64_t)n * cap));
            MK_TRY(c->d_hits.grow((uint64_t)n * std::max(nresults, 1u)));
            MK_TRY(c->d_nhits.grow(n));
            MK_TRY(qset_select(c, v, nresults, cap, c->d_count, c->d_cand, nullptr));
            // the heap over the entrants runs on the device too (K6b): only the hits come back
            MergeArgs ma{c->d_count, c->d_cand, 1, n, cap, nresults, c->d_hits, c->d_nhits};
            MK_TRY(launch_merge(c, ma));
            // results of a small chunk come back through one pinned block (counts, active partitions,
            // hits): three queued copies and ONE wait, instead of a blocking copy per array
            const uint64_t res_bytes = (uint64_t)n * (8 + (uint64_t)nresults * sizeof(mk_hit));
            const bool pinned = res_bytes <= (1ull << 20);
            mk_hit *p_hits = hits + (size_t)q0 * nresults;
            uint32_t *p_nh = nhits + q0, *p_act = act.data() + q0;
            if (pinned) {
                MK_TRY(ensure_pinned(c->h_res, res_bytes + 64));
                p_hits = reinterpret_cast<mk_hit *>(c->h_res.p);
                p_nh = reinterpret_cast<uint32_t *>(c->h_res + (uint64_t)n * nresults * sizeof(mk_hit));
                p_act = p_nh + n;
            }
            MK_HIP(hipMemcpyAsync(p_nh, c->d_nhits, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
            MK_HIP(hipMemcpyAsync(p_act, qs->d_nent + q0, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
            if (nresults)
                MK_HIP(hipMemcpyAsync(p_hits, c->d_hits, (size_t)n * nresults * sizeof(mk_hit), hipMemcpyDeviceToHost, c->stream));
            MK_HIP(hipStreamSynchronize(c->stream));
            if (pinned) {
                memcpy(nhits + q0, p_nh, (size_t)n * 4);
                memcpy(act.data() + q0, p_act, (size_t)n * 4);
                if (nresults) memcpy(hits + (size_t)q0 * nresults, p_hits, (size_t)n * nresults * sizeof(mk_hit));
            }
            // more heap entrants than the device row holds
            for (uint32_t q = q0; q < q1; ++q)
                if (nhits[q] == kMergeOverflow) MK_TRY(replay(q, d_replay_row));
            return MK_OK;
        }, &d_replay_row));
    }
    add_scan_stats(c, act);
    if (active) memcpy(active, act.data(), (size_t)nq * 4);
    return drain_timers(c);                                      // every event has fired: fold them in, keep the list short
}

}  // extern "C"

// ---- query lists: filter_results for any nresults, every genome above the thresholds included (list.hip) ----------------
struct mk_hitlist {
    std::vector<uint64_t> offsets;     // nq + 1
    std::vector<mk_hit> hits;
};

// records a run of queries may leave in the record buffer (8 bytes each; the heaps and the hits of the run are at most
// 12 and 24 bytes per record more).  MIEKKI_LIST_BUDGET_KIB: the tests make chunks take several runs.
static uint64_t list_budget_records()
{
    uint64_t bytes = 256ull << 20;
    if (const char *e = getenv("MIEKKI_LIST_BUDGET_KIB")) { const long v = atol(e); if (v >= 1) bytes = (uint64_t)v << 10; }
    return std::max<uint64_t>(1, bytes / 8);
}

// The per-query host route (replay_query), for the calls the device does not order: NaN intersections
// (nan_candidates_possible).  A dense score row per query, the reference's loop, the host's heap.
static int list_host_rows(mk_ctx *c, mk_qset *qs, uint32_t nresults, bool ordered, uint32_t min_score, double min_inter,
                          std::vector<uint64_t> &off, std::vector<mk_hit> &hits)
{
    MK_TRY(ensure_scores(c, 1));
    std::vector<mk_hit> full;
    for (uint32_t q = 0; q < qs->nq; ++q) {
        MK_TRY(replay_query(c, qs, q, c->d_scores, min_score, min_inter, full));
        const size_t at = hits.size();
        if (!ordered) {
            hits.insert(hits.end(), full.begin(), full.end());
        } else {
            const uint32_t n = (uint32_t)std::min<uint64_t>(nresults, full.size());
            hits.resize(at + n);
            hits.resize(at + mk_filter_candidates(full.data(), (uint32_t)full.size(), n, hits.data() + at));
        }
        off[q + 1] = hits.size();
    }
    return MK_OK;
}

// One pass over a set: off[nq + 1] and the hits of its queries appended to `hits` (off[0] = hits.size() on entry must be 0).
// nresults: any number, MK_ALL_RESULTS, or MK_LIST_CANDIDATES (no heap: the passing genomes in ascending id).
static int qset_run_list(mk_ctx *c, mk_qset *qs, uint32_t nresults, uint32_t min_score, double min_inter,
                         std::vector<uint64_t> &off, std::vector<mk_hit> &hits)
{
    off.assign((size_t)qs->nq + 1, 0);
    hits.clear();
    if (qs->part[0]) {
        // a mixed set: each part runs as a set with its own schedule; the lists go to their queries' places on the host
        std::vector<uint64_t> poff[2];
        std::vector<mk_hit> phits[2];
        for (int i = 0; i < 2; ++i) {
            MK_TRY(qset_run_list(c, qs->part[i], nresults, min_score, min_inter, poff[i], phits[i]));
            for (uint32_t j = 0; j < qs->part[i]->nq; ++j) off[qs->part_q[i][j] + 1] = poff[i][j + 1] - poff[i][j];
        }
        for (uint32_t q = 0; q < qs->nq; ++q) off[q + 1] += off[q];
        hits.resize(off[qs->nq]);
        for (int i = 0; i < 2; ++i)
            for (uint32_t j = 0; j < qs->part[i]->nq; ++j)
                std::copy(phits[i].begin() + poff[i][j], phits[i].begin() + poff[i][j + 1], hits.begin() + off[qs->part_q[i][j]]);
        return MK_OK;
    }
    bool run = false;                                             // (the leaf preamble: stale check, nothing to scan, sketch)
    MK_TRY(qset_leaves(c, qs, [&](mk_qset *, const std::vector<uint32_t> *) { run = true; return (int)MK_OK; }));
    if (!run) return MK_OK;
    const bool ordered = nresults != MK_LIST_CANDIDATES;
    std::vector<uint32_t> act(qs->nq);
    if (nan_candidates_possible(c, min_score)) {
        MK_TRY(list_host_rows(c, qs, nresults, ordered, min_score, min_inter, off, hits));
        MK_HIP(hipMemcpy(act.data(), qs->d_nent, (size_t)qs->nq * 4, hipMemcpyDeviceToHost));
        add_scan_stats(c, act);
        return drain_timers(c);
    }
    mk_ctx::ListScratch &ls = c->list;
    const uint64_t budget = list_budget_records();
    std::vector<uint64_t> h_off;
    // ONE scan per chunk; its scores / partials stay where they are for both passes of every run below
    MK_TRY(for_chunks(c, qs, 0, 1, min_score, min_inter, [&](uint32_t q0, uint32_t q1, const ChunkView &v) -> int {
        const uint32_t n = q1 - q0;
        MK_TRY(ls.d_count.grow(n));
        MK_TRY(ls.d_off.grow(2 * ((uint64_t)n + 1)));
        uint64_t *d_rec_off = ls.d_off, *d_res_off = ls.d_off + ((uint64_t)n + 1);
        ListArgs a = list_args(v, 0, n, ls.d_count, d_rec_off, nullptr);
        {
            ScopedTimer t(c, 2);
            MK_TRY(launch_list_count(c, a));
            MK_TRY(launch_list_scan(c, ls.d_count, n, ordered ? nresults : 0xffffffffu, d_rec_off, d_res_off));
        }
        h_off.resize(2 * ((size_t)n + 1));
        MK_HIP(hipMemcpyAsync(h_off.data(), ls.d_off, h_off.size() * 8, hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipMemcpyAsync(act.data() + q0, qs->d_nent + q0, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        MK_HIP(hipStreamSynchronize(c->stream));
        const uint64_t *rec_off = h_off.data(), *res_off = h_off.data() + n + 1;
        const uint64_t hits0 = hits.size();
        hits.resize(hits0 + res_off[n]);
        for (uint32_t i = 0; i < n; ++i) off[q0 + i + 1] = hits0 + res_off[i + 1];
        // runs of queries whose records fit the budget (a query that exceeds it alone is a run of its own)
        for (uint32_t lo = 0; lo < n;) {
            uint32_t hi = lo + 1;
            while (hi < n && rec_off[hi + 1] - rec_off[lo] <= budget) ++hi;
            const uint64_t nrec = rec_off[hi] - rec_off[lo], nres = res_off[hi] - res_off[lo];
            if (nres) {
                MK_TRY(ls.d_rec.grow(nrec, nrec / 4));
                MK_TRY(ls.d_hits.grow(nres, nres / 4));
                a.q_lo = lo; a.q_n = hi - lo; a.rec = ls.d_rec;
                ScopedTimer t(c, 2);
                MK_TRY(launch_list_write(c, a));
                if (ordered) {
                    const uint64_t nheap = nres + (hi - lo);
                    MK_TRY(ls.d_key.grow(nheap, nheap / 4));
                    MK_TRY(ls.d_ref.grow(nheap, nheap / 4));
                    ListHeapArgs ha{ls.d_rec, d_rec_off, d_res_off, lo, hi - lo, nresults, c->d_sketch_size, c->d_genome_size,
                                    c->p.genome_id_base, ls.d_key, ls.d_ref, ls.d_hits};
                    MK_TRY(launch_list_heap(c, ha));
                } else {
                    MK_TRY(launch_list_expand(c, ls.d_rec, nrec, c->d_sketch_size, c->d_genome_size, c->p.genome_id_base, ls.d_hits));
                }
            }
            if (nres) {
                MK_HIP(hipMemcpyAsync(hits.data() + hits0 + res_off[lo], ls.d_hits, (size_t)nres * sizeof(mk_hit), hipMemcpyDeviceToHost, c->stream));
                MK_HIP(hipStreamSynchronize(c->stream));                // the buffers are the next run's
            }
            lo = hi;
        }
        return MK_OK;
    }));
    add_scan_stats(c, act);
    return drain_timers(c);
}

extern "C" {

int mk_qset_run_list(mk_ctx *c, mk_qset *qs, uint32_t nresults, uint32_t min_score, double min_inter, mk_hitlist **out)
{
    if (!c || !qs || !out) { set_error("null argument"); return MK_ERR_ARG; }
    *out = nullptr;
    MK_TRY(use_device(c));
    std::unique_ptr<mk_hitlist> hl(new mk_hitlist());
    MK_TRY(qset_run_list(c, qs, nresults, min_score, min_inter, hl->offsets, hl->hits));
    *out = hl.release();
    return MK_OK;
}

int mk_query_list(mk_ctx *c, const char *const *seqs, const uint64_t *lens, uint32_t nq, uint32_t nresults, uint32_t min_score,
                  double min_inter, mk_hitlist **out, uint32_t *active)
{
    if (!c || !out || (nq && (!seqs || !lens))) { set_error("null argument"); return MK_ERR_ARG; }
    *out = nullptr;
    MK_TRY(use_device(c));
    std::unique_ptr<mk_hitlist> hl(new mk_hitlist());
    hl->offsets.assign(1, 0);
    // (in slices: a slice's lists go behind those of the slices before it)
    std::vector<uint64_t> off;
    std::vector<mk_hit> hits;
    MK_TRY(for_uploaded_slices(c, seqs, lens, nq, [&](mk_qset *qs, uint32_t q0, uint32_t n) -> int {
        MK_TRY(qset_run_list(c, qs, nresults, min_score, min_inter, off, hits));
        if (active) {
            if (c->G) MK_TRY(mk_qset_active(c, qs, active + q0));
            else memset(active + q0, 0, (size_t)n * 4);                         // no column is ever compared
        }
        const uint64_t base = hl->hits.size();
        for (uint32_t i = 0; i < n; ++i) hl->offsets.push_back(base + off[i + 1]);
        hl->hits.insert(hl->hits.end(), hits.begin(), hits.end());
        return MK_OK;
    }));
    *out = hl.release();
    return MK_OK;
}

const uint64_t *mk_hitlist_offsets(const mk_hitlist *hl) { return hl ? hl->offsets.data() : nullptr; }
const mk_hit *mk_hitlist_hits(const mk_hitlist *hl) { return hl ? hl->hits.data() : nullptr; }
void mk_hitlist_free(mk_hitlist *hl) { delete hl; }

}  // extern "C"

extern "C" {

int mk_exact(mk_ctx *c, const char *const *contigs, const uint64_t *contig_lens, uint32_t n_contigs,
             const char *const *queries, const uint64_t *query_lens, uint32_t nq, uint64_t *inter, uint64_t *uni)
{
    if (!c || (n_contigs && (!contigs || !contig_lens)) || (nq && (!queries || !query_lens || !inter || !uni))) {
        set_error("null argument");
        return MK_ERR_ARG;
    }
    MK_TRY(use_device(c));
    MK_TRY(exact_load_genome(c, contigs, contig_lens, n_contigs));
    return exact_queries(c, queries, query_lens, nq, inter, uni);
}

int mk_exact_load_genome(mk_ctx *c, const char *const *contigs, const uint64_t *contig_lens, uint32_t n_contigs)
{
    if (!c || (n_contigs && (!contigs || !contig_lens))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return exact_load_genome(c, contigs, contig_lens, n_contigs);
}

int mk_exact_query(mk_ctx *c, const char *const *queries, const uint64_t *query_lens, uint32_t nq, uint64_t *inter,
                   uint64_t *uni)
{
    if (!c || (nq && (!queries || !query_lens || !inter || !uni))) { set_error("null argument"); return MK_ERR_ARG; }
    MK_TRY(use_device(c));
    return exact_queries(c, queries, query_lens, nq, inter, uni);
}

}  // extern "C"
