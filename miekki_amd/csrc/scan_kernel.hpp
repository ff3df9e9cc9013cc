// K5 scan kernels (see scan.hip for the design notes).  Kept in a header so that tools/scan_tune.hip can instantiate
// tuning variants of exactly this code, and build its probes from the same pieces.
//
// What the kernels share is written once, ahead of them: a wave's tile of the rows (RowTile), the compare step
// (load_entries, count_ne, list_step), a ranged launch's work numbers and partials (ranged_item, partial_at) and the
// deal of workgroups to the XCDs (xcd_workgroup, xcd_grid).
#pragma once
#include <type_traits>

#include "mk_internal.hpp"

namespace mk {

template <int W>
__device__ __forceinline__ uint32_t bcast_fp(uint32_t fp)
{
    return W == 1 ? fp * 0x01010101u : fp * 0x00010001u;
}

// 1 in the low bit of every byte (half-word) of d that DIFFERS from the query fingerprint: with x = d ^ b and L the low
// seven (fifteen) bits of every byte, (((x & L) + L) | x) >> 7 & 1 per byte.  x is never formed: gfx950's three-input
// v_bitop3_b32 takes the XOR along with the AND and with the OR (truth table bit a << 2 | b << 1 | c: a = 0xf0, b = 0xcc,
// c = 0xaa), so a word costs FIVE vector instructions -- bitop3, add, bitop3, shift, and -- where xor, and, add, or, shift,
// and were six.  The same value bit for bit; every scan kernel compares through here (scan_block_kernel at one byte through
// ne_lanes_block below, four instructions).  (The compiler finds the fused form
// by itself where x has no other use -- scan_block_kernel had it already -- and not in the masked and ragged steps of the
// other kernels, which lose 2-9 % of their vector instructions by it: profiles/r14_scan_block_isa.txt.)
// FUSED = false: x formed once and used twice, as the compiler is then left to arrange it -- scan_group_kernel keeps that
// form, with which it measures 1 % faster (profiles/r14_scan_block_ab.txt, e).
template <int W, bool FUSED = true>
__device__ __forceinline__ uint32_t ne_lanes(uint32_t d, uint32_t b)
{
    constexpr uint32_t LOW = W == 1 ? 0x7f7f7f7fu : 0x7fff7fffu, ONE = W == 1 ? 0x01010101u : 0x00010001u, SHIFT = W == 1 ? 7 : 15;
    if (!FUSED) {
        const uint32_t x = d ^ b;
        return ((((x & LOW) + LOW) | x) >> SHIFT) & ONE;
    }
    const uint32_t t = __builtin_amdgcn_bitop3_b32(d, b, LOW, 0x28);         // (d ^ b) & L
    const uint32_t y = t + LOW;
    const uint32_t z = __builtin_amdgcn_bitop3_b32(d, b, y, 0xbe);           // (d ^ b) | y
    return (z >> SHIFT) & ONE;
}

// The same flags for scan_block_kernel alone (the other kernels keep ne_lanes, instruction for instruction).  At one byte
// FOUR instructions: v_lerp_u8 x, 0xff, 0 is (x + 255) >> 1 in every byte with no carry between bytes, and bit 7 of that is
// set exactly when x != 0 -- xor, lerp, shift, and.  (v_lerp_u8 issues in 4.6 cycles at four waves per SIMD where the
// others take about 3: the step is 2 % shorter for it, profiles/r15_scan_block_ab.txt.)  At two bytes ne_lanes: xor and
// v_pk_min_u16 (x, 1), two instructions where five stand, measured 5 % SLOWER on the two-byte shape and is not built.
template <int W>
__device__ __forceinline__ uint32_t ne_lanes_block(uint32_t d, uint32_t b)
{
    if (W != 1) return ne_lanes<W>(d, b);
    return (__builtin_amdgcn_lerp(d ^ b, 0xffffffffu, 0u) >> 7) & 0x01010101u;
}

template <bool NT>
__device__ __forceinline__ uint4 load_row16(const uint8_t *p)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    if (NT) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const uint4 *>(p);
}

// Address of the wave's tile of row p as a SCALAR base (SALU multiply-add, kept in
// SGPRs through readfirstlane) so that the load is the saddr form
// `global_load_dwordx4 v, v_off, s[base]` with one 32-bit per-lane offset.
__device__ __forceinline__ const uint8_t *row_base(const uint8_t *base, uint32_t p, uint64_t ld)
{
    const uint64_t roff = (uint64_t)p * ld;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)roff);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(roff >> 32));
    return base + (((uint64_t)hi << 32) | lo);
}

// the same with the row's home chosen first: rows below P_hot in HBM, the rest in (device-visible)
// host memory (MatRef).  p is wave-uniform, so the choice is scalar arithmetic too.
__device__ __forceinline__ const uint8_t *row_base(const uint8_t *hot, const uint8_t *cold, uint32_t P_hot, uint32_t p,
                                                   uint64_t ld)
{
    const uint32_t pu = __builtin_amdgcn_readfirstlane(p);
    return row_base(pu < P_hot ? hot : cold, pu, ld);
}

// Per LANE (a vector address): narrow tiles, where a wave-instruction covers several rows (scan_block_kernel).  The lane's
// bytes of row `rel` of a partition range, from the lane's bytes of the range's first row in the range's home: ONE 32 x 32-bit
// multiply-add onto a 64-bit base that holds everything else (the launch checks that the pitch fits 32 bits, and that
// no range of the launch has rows in both homes).
__device__ __forceinline__ const uint8_t *piece_base(const uint8_t *first, uint32_t rel, uint32_t ld)
{
    return first + (uint64_t)rel * ld;
}

// where the rows from P_hot on live: a matrix without cold rows has them all in HBM
__device__ __forceinline__ const uint8_t *cold_home(const uint8_t *M, const uint8_t *Mc) { return Mc ? Mc : M; }

// A wave's 1 KiB tile of the rows: the tile's first byte of row 0 in either home, and the lane's 16 bytes of it.
struct RowTile {
    const uint8_t *hot, *cold;
    uint64_t ld;
    uint32_t P_hot, voff;
    template <bool NT>
    __device__ __forceinline__ uint4 load(uint32_t p) const { return load_row16<NT>(row_base(hot, cold, P_hot, p, ld) + voff); }
    // this lane has genomes in the tile: the others retire at once, so a row's last tile only fetches what it needs
    template <int W>
    static __device__ __forceinline__ bool live(uint32_t tile, uint32_t lane, uint32_t G)
    {
        return (uint64_t)tile * kTileBytes + lane * 16u < (uint64_t)G * W;
    }
};

template <typename Args>   // ScanArgs, SlabArgs, DenseArgs
__device__ __forceinline__ RowTile row_tile(const Args &a, uint32_t tile, uint32_t lane)
{
    return RowTile{a.M + (uint64_t)tile * kTileBytes, cold_home(a.M, a.Mc) + (uint64_t)tile * kTileBytes, a.ld, a.P_hot, lane * 16u};
}

// ---------------------------------------------------------------- one compare step
// UNROLL entries of a (wave-uniform) list: their rows' 16-byte loads issued back to back, before the first use -- eight
// (four) in flight per wave -- then each row's four words compared with its entry's fingerprint into packed counters.
// TAIL: the ragged last step of a list of m entries, still UNROLL loads in flight: the spare slots re-read the last
// entry (cached) and are masked out of the sums -- branch-free, one memory latency instead of one per entry.
template <int UNROLL, bool TAIL>
__device__ __forceinline__ void load_entries(uint64_t (&ev)[UNROLL], const uint64_t *__restrict__ e, uint32_t j, uint32_t m)
{
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) ev[u] = e[TAIL ? min(j + u, m - 1) : j + u];
}

__device__ __forceinline__ uint32_t tail_keep(uint32_t j, int u, uint32_t m) { return j + u < m ? 0xffffffffu : 0u; }   // wave-uniform

// MASK: counted only where keep is all ones (the steps that count everything do not pay for the AND).
template <int W, bool MASK, bool FUSED = true>
__device__ __forceinline__ uint4 count_ne(uint4 acc, const uint4 &d, uint32_t b, uint32_t keep = 0xffffffffu)
{
    acc.x += MASK ? ne_lanes<W, FUSED>(d.x, b) & keep : ne_lanes<W, FUSED>(d.x, b);
    acc.y += MASK ? ne_lanes<W, FUSED>(d.y, b) & keep : ne_lanes<W, FUSED>(d.y, b);
    acc.z += MASK ? ne_lanes<W, FUSED>(d.z, b) & keep : ne_lanes<W, FUSED>(d.z, b);
    acc.w += MASK ? ne_lanes<W, FUSED>(d.w, b) & keep : ne_lanes<W, FUSED>(d.w, b);
    return acc;
}

// A step of a list e[0, m) from entry j on.  WINDOW: only the entries whose partition lies in [wlo, wlo + wspan) count,
// n_in counts them; a full step with none in the window is skipped by a scalar branch, a step with some loads the
// window's first row for the others (cached).  The forms -- full, windowed, ragged -- differ in which entries they keep.
template <int W, int UNROLL, bool NT, bool WINDOW, bool TAIL>
__device__ __forceinline__ void list_step(uint4 &acc, const RowTile &t, const uint64_t *__restrict__ e, uint32_t j, uint32_t m,
                                           uint32_t wlo, uint32_t wspan, uint32_t &n_in)
{
    uint64_t ev[UNROLL];
    uint32_t keep[UNROLL], any = 0;
    load_entries<UNROLL, TAIL>(ev, e, j, m);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        keep[u] = TAIL ? tail_keep(j, u, m) : 0xffffffffu;
        if (WINDOW) {
            if (((uint32_t)ev[u] - wlo) >= wspan) keep[u] = 0u;
            any |= keep[u];
            n_in += keep[u] & 1u;
        }
    }
    if (WINDOW && !TAIL && !__builtin_amdgcn_readfirstlane(any)) return;
    uint4 d[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) d[u] = t.load<NT>((!WINDOW || keep[u]) ? (uint32_t)ev[u] : wlo);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) acc = count_ne<W, WINDOW || TAIL>(acc, d[u], bcast_fp<W>((uint32_t)(ev[u] >> 32)), keep[u]);
}

// the whole list (at most as many entries as packed counters hold): full steps, then the ragged one
template <int W, int UNROLL, bool NT, bool WINDOW>
__device__ __forceinline__ uint4 compare_list(const RowTile &t, const uint64_t *__restrict__ e, uint32_t m, uint32_t wlo, uint32_t wspan,
                                              uint32_t &n_in)
{
    uint4 acc = make_uint4(0, 0, 0, 0);
    uint32_t j = 0;
    for (; j + UNROLL <= m; j += UNROLL) list_step<W, UNROLL, NT, WINDOW, false>(acc, t, e, j, m, wlo, wspan, n_in);
    if (j < m) list_step<W, UNROLL, NT, WINDOW, true>(acc, t, e, j, m, wlo, wspan, n_in);
    return acc;
}

// the same with every entry counting (no window)
template <int W, int UNROLL>
__device__ __forceinline__ uint4 compare_list(const RowTile &t, const uint64_t *__restrict__ e, uint32_t m)
{
    uint32_t all = 0;
    return compare_list<W, UNROLL, false, false>(t, e, m, 0u, 0u, all);
}

// One work item: query `ql` of the launch against row tile `tile`.
// WINDOW: only the entries whose partition lies in [a.row_lo, a.row_hi) count -- the launch covers one window
// of rows (the part of the matrix in HBM, or a cold range staged there: api_query.hip, scan_windows) and ADDS its
// share to the scores when a.accumulate is set.
template <int W, int UNROLL, bool NT, bool WINDOW = false>
__device__ __forceinline__ void scan_item(const ScanArgs &a, uint32_t ql, uint32_t tile, uint32_t lane)
{
    constexpr uint32_t NCNT = 16 / W;                    // genomes per lane
    constexpr uint32_t CHUNK = W == 1 ? 255u : 65535u;   // entries before packed counters overflow
    if (!RowTile::live<W>(tile, lane, a.G)) return;
    const uint32_t q = a.q_begin + ql;
    const uint64_t *__restrict__ ent = a.entries + a.ent_off[q];
    const uint32_t n = a.nent[q];
    const RowTile t = row_tile(a, tile, lane);

    uint32_t ne32[NCNT];
#pragma unroll
    for (uint32_t j = 0; j < NCNT; ++j) ne32[j] = 0;
    uint32_t n_in = WINDOW ? 0u : n;                                 // entries that count (wave-uniform)
    const uint32_t wlo = a.row_lo, wspan = a.row_hi - a.row_lo;

    for (uint32_t i0 = 0; i0 < n; i0 += CHUNK) {
        const uint32_t m = min(n - i0, CHUNK);
        const uint64_t *__restrict__ e = ent + i0;
        const uint4 acc = compare_list<W, UNROLL, NT, WINDOW>(t, e, m, wlo, wspan, n_in);
        const uint32_t wide[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            if (W == 1) {
                ne32[4 * w + 0] += wide[w] & 0xffu;
                ne32[4 * w + 1] += (wide[w] >> 8) & 0xffu;
                ne32[4 * w + 2] += (wide[w] >> 16) & 0xffu;
                ne32[4 * w + 3] += wide[w] >> 24;
            } else {
                ne32[2 * w + 0] += wide[w] & 0xffffu;
                ne32[2 * w + 1] += wide[w] >> 16;
            }
        }
    }

    // shared fingerprints = active entries - differing ones
    const uint32_t g0 = tile * (kTileBytes / W) + lane * NCNT;
    uint32_t score[NCNT];
#pragma unroll
    for (uint32_t j = 0; j < NCNT; ++j) score[j] = n_in - ne32[j];

    // scores[tile * score_tile_stride + ql * score_q_stride + genome-in-tile]: row-major
    // ([query][genome], q_stride = row pitch, tile_stride = genomes per tile) for callers
    // that want dense rows, tile-major ([tile][query][genomes per tile]) for the
    // pipeline -- there consecutive waves store consecutive 4 KiB pieces, a pure stream
    if (!a.scores) {                                                   // store-less timing runs (tools/scan_tune)
#pragma unroll
        for (uint32_t j = 0; j < NCNT; ++j) asm volatile("" ::"v"(score[j]));   // keep the compare loop live
        return;
    }
    uint32_t *__restrict__ row = a.scores + (uint64_t)tile * a.score_tile_stride + (uint64_t)ql * a.score_q_stride;
    const uint32_t i0 = lane * NCNT;                                   // genome index inside the tile
    if (WINDOW && a.accumulate) {                                      // a later window of the same launch sequence: this
        if (n_in == 0) return;                                         // wave owns the same words in every window, in stream order
        if (a.score_vec) {
#pragma unroll
            for (uint32_t j = 0; j < NCNT; j += 4) {
                uint4 v = *reinterpret_cast<uint4 *>(row + i0 + j);
                v.x += score[j]; v.y += score[j + 1]; v.z += score[j + 2]; v.w += score[j + 3];
                *reinterpret_cast<uint4 *>(row + i0 + j) = v;
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < NCNT; ++j)
                if (g0 + j < a.G) row[i0 + j] += score[j];
        }
        return;
    }
    if (a.score_vec) {
#pragma unroll
        for (uint32_t j = 0; j < NCNT; j += 4)
            *reinterpret_cast<uint4 *>(row + i0 + j) = make_uint4(score[j], score[j + 1], score[j + 2], score[j + 3]);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < NCNT; ++j)
            if (g0 + j < a.G) row[i0 + j] = score[j];
    }
}

// ORDER 0: consecutive waves take adjacent tiles of one query (query-major);
// ORDER 1: consecutive waves take the same tile of consecutive queries (tile-major).
// NT: non-temporal row loads.
template <int W, int UNROLL, int ORDER = 1, bool NT = false, bool WINDOW = false>
__global__ __launch_bounds__(256) void scan_kernel(const ScanArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t work = blockIdx.x * 4u + wave;
    if (work >= a.nq * a.ntiles) return;                 // wave-uniform exit
    uint32_t ql, tile;
    if (ORDER == 0) { ql = work / a.ntiles; tile = work - ql * a.ntiles; }
    else            { tile = work / a.nq;   ql = work - tile * a.nq; }
    scan_item<W, UNROLL, NT, WINDOW>(a, ql, tile, lane);
}

// ---------------------------------------------------------------- ranged launches (SlabArgs: slab, group and block kernels)
// The partitions are cut into S ranges; a launch walks ranges [r_begin, r_begin + r_count) of every tile.  Work number
// `work` of a launch with n items per (tile, range), the items running fastest, then the ranges: item x of (tile, r).
struct RangedItem { uint32_t tile, r, tr, x; };   // tr: the (tile, range)'s place in the partials

__device__ __forceinline__ RangedItem ranged_item(const SlabArgs &a, uint32_t work, uint32_t n)
{
    const uint32_t trl = work / n, x = work - trl * n;
    const uint32_t tile = trl / a.r_count, r = a.r_begin + (trl - tile * a.r_count);
    return RangedItem{tile, r, tile * a.S + r, x};
}

// the 1 KiB PARTIAL of (tile, range) tr and query ql of the launch: [tile][range][query][1 KiB]
__device__ __forceinline__ uint8_t *partial_at(const SlabArgs &a, uint32_t tr, uint32_t ql)
{
    return a.partials + ((uint64_t)tr * a.nq + ql) * kTileBytes;
}

// ---------------------------------------------------------------- dealing workgroups to the XCDs
// The hardware hands workgroup b to XCD b % 8.  A kernel that wants the workgroups in flight on one XCD to be
// NEIGHBOURS in its own numbering (they share rows or tables through that XCD's L2) takes this number instead of
// blockIdx.x: XCD x walks the x-th eighth of the numbers in order.  The grid must be a multiple of eight workgroups
// -- xcd_grid -- and the kernel lets the numbers past its work go.
__device__ __forceinline__ uint32_t xcd_workgroup()
{
    const uint32_t per_xcd = gridDim.x / 8u;
    return (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
}
inline uint32_t xcd_grid(uint32_t workgroups) { return (workgroups + 7u) / 8u * 8u; }

// ---------------------------------------------------------------- slab schedule
// A work item is (tile, range, query), ordered tile-major then range-major: the waves in flight share one
// (2^h / S) x 1 KiB slab of the matrix, sized by the host to fit the Infinity
// Cache, so a row piece is fetched from HBM about once and then re-read on die by
// the other queries that need it (measured: 6.65 -> 8.0 TB/s at 1/8 of 2^20 rows).
// A (query, range) has at most 255 entries (65,535 at 2 bytes) -- the host checks --
// so the packed per-genome mismatch counters never overflow and are simply stored,
// 16 bytes per lane, as this range's PARTIAL: no read-modify-write, no ordering
// between ranges.  select.hip sums the S partials of a genome.
template <int W, int UNROLL>
__global__ __launch_bounds__(256) void scan_slab_kernel(const SlabArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t work = blockIdx.x * 4u + wave;
    if (work >= a.ntiles * a.r_count * a.nq) return;     // wave-uniform exit
    const RangedItem it = ranged_item(a, work, a.nq);
    const uint32_t ql = it.x, r = it.r;
    if (!RowTile::live<W>(it.tile, lane, a.G)) return;
    const uint32_t q = a.q_begin + ql;
    uint32_t lo, hi;
    if (a.kind == RangedScan::ByCount) {                // small sets: ranges by entry COUNT (no range table, no eligibility check)
        const uint32_t n = a.nent[q];
        lo = min(r * a.chunk, n);
        hi = min(lo + a.chunk, n);
    } else {
        lo = a.split[(uint64_t)q * (a.S + 1) + r];
        hi = a.split[(uint64_t)q * (a.S + 1) + r + 1];
    }
    const uint64_t *__restrict__ e = a.entries + a.ent_off[q] + lo;
    const uint32_t m = hi - lo;
    const RowTile t = row_tile(a, it.tile, lane);
    *reinterpret_cast<uint4 *>(partial_at(a, it.tr, ql) + t.voff) = compare_list<W, UNROLL>(t, e, m);
}

// ---------------------------------------------------------------- query groups
// scan_slab_kernel keeps ONE query's counters per wave: about 1,024 queries are in flight per XCD, and a row piece
// (partition, 1 KiB tile) is wanted by fewer than one of them while it sits in L2 -- every compared byte comes from
// the Infinity Cache.  Here a wave carries QW consecutive queries (a GROUP) against one (tile, range): QW x 4 VGPRs
// of packed counters, and ONE merged entry list, ordered by (window, slot, partition), where a window is a band of
// 2^wshift partitions of the range.  The waves in flight on an XCD (dispatch order: scan_group_kernel) walk the
// same (tile, range) window by window, so a row piece fetched into L2 is read by several queries before it leaves.
// A list entry is the query's entry with its slot in the group in bits 48..63: partition | (fp | slot << 16) << 32.
// The list of (group g, range r) lies at entries_of_group(g) + sum over the group's queries q of split[q][r]: the
// group's lists fill exactly the room its queries' entry lists have (ent_off), range after range.

struct GroupArgs {
    const uint64_t *entries;       // [ent_off[q] ...] per query, ascending partition
    const uint64_t *ent_off;
    const uint32_t *split;         // [query][S + 1]
    uint64_t *lists;               // out: the groups' merged lists (same room as entries)
    uint32_t nq, S, P, wshift, nwin;
};

template <int QW>
__global__ __launch_bounds__(256) void group_list_kernel(const GroupArgs a)
{
    __shared__ uint32_t s_cnt[kGroupCells], s_first[kGroupCells];
    __shared__ uint32_t s_part[256];
    const uint32_t g = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const uint32_t ncell = a.nwin * QW;
    for (uint32_t c = tid; c < ncell; c += 256) { s_cnt[c] = 0; s_first[c] = 0xffffffffu; }
    __syncthreads();
    const uint32_t q0 = g * QW, rlo = r * (a.P / a.S);
    uint64_t dst = a.ent_off[q0];
    uint32_t lo[QW], n[QW];
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)QW; ++s) {
        const uint32_t q = q0 + s;
        lo[s] = q < a.nq ? a.split[(uint64_t)q * (a.S + 1) + r] : 0u;
        n[s] = q < a.nq ? a.split[(uint64_t)q * (a.S + 1) + r + 1] - lo[s] : 0u;
        dst += lo[s];
    }
    auto cell_of = [&](uint32_t s, uint64_t e) { return min(((uint32_t)e - rlo) >> a.wshift, a.nwin - 1u) * QW + s; };
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)QW; ++s) {
        const uint64_t *__restrict__ e = a.entries + a.ent_off[min(q0 + s, a.nq - 1u)] + lo[s];
        for (uint32_t i = tid; i < n[s]; i += 256) {
            const uint32_t c = cell_of(s, e[i]);
            atomicAdd(&s_cnt[c], 1u);
            atomicMin(&s_first[c], i);
        }
    }
    __syncthreads();
    // exclusive scan of the cell counts: each thread a run of cells, then the runs' sums
    const uint32_t per = (ncell + 255) / 256, c0 = tid * per, c1 = min(c0 + per, ncell);
    uint32_t sum = 0;
    for (uint32_t c = c0; c < c1; ++c) sum += s_cnt[c];
    s_part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (uint32_t t = 0; t < 256; ++t) { const uint32_t v = s_part[t]; s_part[t] = run; run += v; }
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (uint32_t c = c0; c < c1; ++c) { const uint32_t v = s_cnt[c]; s_cnt[c] = run; run += v; }
    __syncthreads();
    uint64_t *__restrict__ out = a.lists + dst;
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)QW; ++s) {
        const uint64_t *__restrict__ e = a.entries + a.ent_off[min(q0 + s, a.nq - 1u)] + lo[s];
        for (uint32_t i = tid; i < n[s]; i += 256) {
            const uint64_t v = e[i];
            const uint32_t c = cell_of(s, v);
            out[s_cnt[c] + (i - s_first[c])] = v | ((uint64_t)s << 48);
        }
    }
}

// One wave: (tile, range, group of QW queries).  Workgroups are dealt to the eight XCDs (xcd_workgroup): XCD x
// takes the x-th eighth of the work in order, whose numbers run (tile, range)-major with the group fastest, so the waves
// in flight on one XCD are the groups of one or two (tile, range) pairs, walking their windows at about the same pace.
// (Nothing waits on anything: the order buys speed, never correctness.)  Every (tile, range, query) partial of the launch
// is stored, zeros included, exactly as scan_slab_kernel stores it.
template <int W, int QW, int UNROLL>
__global__ __launch_bounds__(256) void scan_group_kernel(const SlabArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t work = xcd_workgroup() * 4u + wave;
    // groups of the launch: set groups g_begin .. g_begin + ngroups - 1 (the first and last may reach outside
    // [q_begin, q_begin + nq): their other slots are compared along and not stored)
    const uint32_t g_begin = a.q_begin / QW, ngroups = (a.q_begin + a.nq - 1) / QW - g_begin + 1;
    if (work >= a.ntiles * a.r_count * ngroups) return;                  // wave-uniform exit
    const RangedItem it = ranged_item(a, work, ngroups);
    const uint32_t g = g_begin + it.x, r = it.r;
    if (!RowTile::live<W>(it.tile, lane, a.G)) return;
    const uint32_t nq_set = a.nset, q0 = g * QW;
    uint64_t lo = a.ent_off[q0], hi = lo;
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)QW; ++s) {
        if (q0 + s >= nq_set) break;
        lo += a.split[(uint64_t)(q0 + s) * (a.S + 1) + r];
        hi += a.split[(uint64_t)(q0 + s) * (a.S + 1) + r + 1];
    }
    const uint64_t *__restrict__ e = a.lists + lo;
    const uint32_t m = (uint32_t)(hi - lo);
    const RowTile t = row_tile(a, it.tile, lane);
    // the group's counters (a query's per-range count fits them: the host checks <= 255 / 65,535 entries)
    uint32_t cnt[QW][4];
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)QW; ++s) cnt[s][0] = cnt[s][1] = cnt[s][2] = cnt[s][3] = 0;
    // a run of one slot's entries is summed in acc and added to that slot's counters when the slot changes: a
    // wave-uniform switch over constant indices (the counters stay in registers, no indexed access)
    uint32_t cur = 0;
    uint4 acc = make_uint4(0, 0, 0, 0);
    auto flush = [&]() {
#pragma unroll
        for (uint32_t s = 0; s < (uint32_t)QW; ++s)
            if (cur == s) { cnt[s][0] += acc.x; cnt[s][1] += acc.y; cnt[s][2] += acc.z; cnt[s][3] += acc.w; }
        acc = make_uint4(0, 0, 0, 0);
    };
    for (uint32_t j = 0; j < m; j += UNROLL) {                            // (every step in the ragged form)
        uint64_t ev[UNROLL];
        uint4 d[UNROLL];
        load_entries<UNROLL, true>(ev, e, j, m);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) d[u] = t.load<false>((uint32_t)ev[u]);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t hi32 = __builtin_amdgcn_readfirstlane((uint32_t)(ev[u] >> 32));
            const uint32_t slot = hi32 >> 16;
            if (slot != cur) { flush(); cur = slot; }
            // (the compare in its unfused form: this kernel is 1 % slower with the fused one, profiles/r14_scan_block_ab.txt)
            acc = count_ne<W, true, false>(acc, d[u], bcast_fp<W>(hi32 & 0xffffu), tail_keep(j, u, m));
        }
    }
    flush();
#pragma unroll
    for (uint32_t s = 0; s < (uint32_t)QW; ++s) {
        const uint32_t q = q0 + s;
        if (q < a.q_begin || q >= a.q_begin + a.nq) continue;             // wave-uniform
        *reinterpret_cast<uint4 *>(partial_at(a, it.tr, q - a.q_begin) + t.voff) = make_uint4(cnt[s][0], cnt[s][1], cnt[s][2], cnt[s][3]);
    }
}

// ---------------------------------------------------------------- query blocks
// The group kernel fetches a row piece once per query that wants it: the counters of the queries that share a piece must
// sit in one CU, a CU's registers hold 256 queries' counters at a 1 KiB tile, and 256 x 908 / 2^20 = 0.22 of them want a
// given row.  Here a BLOCK of B consecutive queries of the set is counted in LDS against a T-byte sub-tile of the 1 KiB
// tile: B x T bytes of packed counters (B = 1,280 at T = 128: all 160 KiB), so that 1.11 queries of the block want a touched
// row piece and the piece is loaded ONCE for all of them -- by construction, inside one workgroup, whatever runs beside it.
// A (block, range) has a list GROUPED BY PARTITION, in 16-byte PACKETS: a row record -- the partition (from the range's
// first) and a count, in one word -- and up to three of the partition's PAIR WORDS (slot in block, fingerprint), written by
// block_list_kernel in the form scan_block_kernel, their only reader, consumes (pair_word below):
//   one-byte fingerprints   fingerprint << 24 | BYTE OFFSET of the slot's counters in LDS (slot x pitch, 24 bits)
//   two-byte fingerprints   slot << 16 | fingerprint (the fingerprint leaves no room for an offset)
// A partition that more than three queries of the block want has several packets.  A group of T / 16 lanes takes a packet
// (one 4-byte load per lane: a wave's eight packets are 128 contiguous bytes), loads its 16 bytes per lane of the row piece
// -- a per-lane address, 1024 / T rows per wave-instruction -- and adds the SWAR compare of every pair of the packet to the
// pair's slot with LDS integer adds (64-bit: two counter words each).  Integer adds commute and a (query, range) has at
// most 255 (65,535) entries, so no counter carries into its neighbour: the partials are bit for bit scan_slab_kernel's, in
// whatever order the adds land.
struct BlockListArgs {
    const uint64_t *entries;       // [ent_off[q] ...] per query, ascending partition
    const uint64_t *ent_off;
    const uint32_t *split;         // [query][S + 1]
    uint4 *packets;                // out: x = partition - range's first | pairs << 24, y z w = the pair words
    BlockInfo *info;               // out: [block][S]
    uint32_t nq, S, P, B;
    uint32_t W, pitch;             // what a pair word holds: the fingerprint width, and the bytes from a slot's counters to the next's
};

constexpr uint32_t kBlockWindow = 1024;   // partitions sorted at a time (one LDS bin each)
// queries per block at most: three per thread of block_list_kernel.  (A pair word has 24 bits for the byte offset of the
// last slot's counters, 16 for the slot itself at two-byte fingerprints: 3,072 slots of up to 4 KiB fit both.)
constexpr uint32_t kBlockMaxB = 3072;
constexpr uint32_t kPacketPairs = 3;

// The pair word of (slot, fingerprint), and what scan_block_kernel takes out of it.  PITCH: bytes from slot to slot.
template <int W>
__device__ __forceinline__ uint32_t pair_word(uint32_t slot, uint32_t fp, uint32_t pitch)
{
    return W == 1 ? (fp << 24) | (slot * pitch) : (slot << 16) | (fp & 0xffffu);
}
// the fingerprint in every byte (half-word) of a word: one v_perm_b32 (selector byte i names the byte that lands in byte i)
template <int W>
__device__ __forceinline__ uint32_t pair_fp(uint32_t pw)
{
    return __builtin_amdgcn_perm(pw, pw, W == 1 ? 0x03030303u : 0x01000100u);
}
// the byte offset in LDS of the lane's four counter words of the pair's slot; l16: the lane's 16 l inside the slot's counters.
// At W = 1 one v_and_or_b32 (the slot's offset is a multiple of PITCH = T, a power of two above l16), at W = 2 a shift and a
// shift-add.
template <int W, uint32_t PITCH>
__device__ __forceinline__ uint32_t pair_offset(uint32_t pw, uint32_t l16)
{
    static_assert((PITCH & (PITCH - 1)) == 0, "the lane's offset is OR-ed into the slot's");
    return W == 1 ? (pw & 0xffffffu) | l16 : (pw >> 16) * PITCH + l16;
}

// sums of v over the threads before this one in the workgroup of 1,024 (exclusive) and over all of them; s_w: 16 words
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t v, uint32_t *s_w, uint32_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                                   // (s_w free again)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) { const uint32_t t = s_w[w]; all += t; if (w < wave) before += t; }
    total = all;
    return before + inc - v;
}

// One workgroup per (block, range): a two-level counting sort.  Every query's entries of the range are ascending, so the
// first level -- the window of 1,024 partitions an entry falls into -- is a cursor per query that moves on window by window;
// the second is a histogram of the window's 1,024 partitions in LDS.  A partition with c pairs has c / 3 full packets and one
// of c % 3; a window's packets are laid down BY PAIR COUNT -- those of one pair, of two, of three -- behind the windows
// before, so that the lane groups of a wave, which take consecutive packets, mostly have equally many pairs to count (the
// order of the rows inside a window is free: 1,024 rows of one tile are a quarter of an XCD's L2).  A pair is written as the
// pair word of its width (pair_word: fingerprint << 24 | slot x a.pitch at one byte, slot << 16 | fingerprint at two), so
// the lists of a set belong to the width and the slot pitch they were made for.
__global__ __launch_bounds__(1024) void block_list_kernel(const BlockListArgs a)
{
    __shared__ uint32_t s_hist[kBlockWindow], s_rest[kBlockWindow], s_full[kBlockWindow], s_fill[kBlockWindow], s_w[16];
    constexpr uint32_t OWN = kBlockMaxB / 1024;
    const uint32_t b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const uint32_t q0 = b * a.B, rlo = r * (a.P / a.S), rhi = r + 1 == a.S ? a.P : rlo + a.P / a.S;
    const uint64_t *e[OWN];
    uint32_t cur[OWN], end[OWN], stop[OWN];
    uint32_t lo_sum = 0, n_sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < OWN; ++k) {
        const uint32_t s = tid + k * 1024u, q = q0 + s;
        const bool on = s < a.B && q < a.nq;
        e[k] = a.entries + a.ent_off[on ? q : 0];
        cur[k] = on ? a.split[(uint64_t)q * (a.S + 1) + r] : 0u;
        end[k] = on ? a.split[(uint64_t)q * (a.S + 1) + r + 1] : 0u;
        lo_sum += cur[k]; n_sum += end[k] - cur[k];
    }
    // (the block's lists fill the room its queries' entry lists have, range after range, as the groups' do -- a packet per
    // pair at most; the sums stay below 2^32: a block's queries are short ones)
    uint32_t lo_all, npairs;
    block_scan_1024(lo_sum, s_w, lo_all);
    block_scan_1024(n_sum, s_w, npairs);
    const uint64_t base = a.ent_off[q0] + lo_all + ((uint64_t)b * a.S + r) * kBlockStepPackets;
    uint4 *__restrict__ pk = a.packets + base;
    uint32_t *__restrict__ pkw = reinterpret_cast<uint32_t *>(pk);
    uint32_t pair_run = 0, pk_run = 0;
    for (uint32_t wlo = rlo; wlo < rhi && pair_run < npairs; wlo += kBlockWindow) {
        const uint32_t span = min(kBlockWindow, rhi - wlo);
        s_hist[tid] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < OWN; ++k) {
            uint32_t i = cur[k];
            for (; i < end[k]; ++i) {
                const uint32_t off = (uint32_t)e[k][i] - wlo;
                if (off >= span) break;
                atomicAdd(&s_hist[off], 1u);
            }
            stop[k] = i;
        }
        __syncthreads();
        const uint32_t c = s_hist[tid], nfull = c / kPacketPairs, rest = c - nfull * kPacketPairs;
        uint32_t wpairs, t12, t3;
        block_scan_1024(c, s_w, wpairs);
        const uint32_t r12 = block_scan_1024((rest == 1 ? 1u : 0u) | (rest == 2 ? 0x10000u : 0u), s_w, t12);
        const uint32_t r3 = block_scan_1024(nfull, s_w, t3);
        const uint32_t t1 = t12 & 0xffffu, t2 = t12 >> 16;
        const uint32_t at_rest = pk_run + (rest == 1 ? r12 & 0xffffu : t1 + (r12 >> 16)), at_full = pk_run + t1 + t2 + r3;
        const uint32_t relp = wlo + tid - rlo;
        if (rest) pkw[(uint64_t)at_rest * 4] = relp | (rest << 24);
        for (uint32_t i = 0; i < nfull; ++i) pkw[(uint64_t)(at_full + i) * 4] = relp | (kPacketPairs << 24);
        s_rest[tid] = at_rest; s_full[tid] = at_full; s_fill[tid] = 0;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < OWN; ++k) {
            const uint32_t slot = tid + k * 1024u;
            for (uint32_t i = cur[k]; i < stop[k]; ++i) {
                const uint64_t v = e[k][i];
                const uint32_t bin = (uint32_t)v - wlo;
                const uint32_t j = atomicAdd(&s_fill[bin], 1u), full = s_hist[bin] / kPacketPairs * kPacketPairs;
                const uint32_t at = j < full ? s_full[bin] + j / kPacketPairs : s_rest[bin];
                const uint32_t w = j < full ? j % kPacketPairs : j - full;
                const uint32_t fp = (uint32_t)(v >> 32) & 0xffffu;
                pkw[(uint64_t)at * 4 + 1 + w] = a.W == 1 ? pair_word<1>(slot, fp, a.pitch) : pair_word<2>(slot, fp, a.pitch);
            }
            cur[k] = stop[k];
        }
        pair_run += wpairs; pk_run += t1 + t2 + t3;
        __syncthreads();
    }
    // zero packets up to a whole step: each costs scan_block_kernel one (cached) row load and no pair block, and its loop
    // needs no test against the list's end (0.3 % more packets at 100,000 queries of 1 kb)
    const uint32_t padded = (pk_run + kBlockStepPackets - 1) / kBlockStepPackets * kBlockStepPackets;
    for (uint32_t i = pk_run + tid; i < padded; i += 1024) pk[i] = make_uint4(0, 0, 0, 0);
    if (tid == 0) a.info[(uint64_t)b * a.S + r] = BlockInfo{base, npairs, padded};
}

// word K of the lane's quad (lanes 4i .. 4i + 3), in every lane of the quad: one v_mov_b32 with a DPP quad_perm
template <int K>
__device__ __forceinline__ uint32_t quad_word(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, K * 0x55, 0xf, 0xf, true);
}

// One workgroup of sixteen waves: (tile, range, block, T-byte sub-tile), numbered (tile, range)-major and dealt to the XCDs
// (xcd_workgroup).  Within a (tile, range) a run of F = a.block_sub_fast consecutive sub-tiles varies fastest, then the block,
// then the NSUB / F runs: F = NSUB is sub-tile fastest (an XCD's 32 workgroups in flight are 4 blocks on each of 8 sub-tiles),
// F = 1 is block fastest (up to 32 blocks on one sub-tile, the only workgroups that can want the same row piece) and what the
// host asks for (kBlockSubFast: a third of the bytes across the fabric, 12 % off the step -- DESIGN.md 4.1, round 13).  The order
// is an argument, not a template parameter: it is a few scalar instructions ahead of the first barrier, and the packet loop
// is the same code for every F (profiles/r13_scan_block_order_isa.txt).  Blocks are the SET's (block b = its queries
// [b B, (b + 1) B)): the first and last block of a launch may reach outside [q_begin, q_begin + nq), their other slots are
// counted along and not stored.  Every (tile, range, query) partial of the launch is stored, zeros included, exactly where
// scan_slab_kernel stores it.  No workgroup waits for another.
//
// The packet loop has no guards: the lists are whole steps (block_list_kernel pads them with zero packets) and the lanes past
// the last genome load live bytes and add into cells that are never stored, so a step is about 9 vector instructions per
// packet -- four DPP moves, the AND and multiply-add of the row address, three compares of the pair count -- and the pair blocks.
// The ORDER in which a step's requests leave and are waited for is stated, not left to the compiler (sched_barrier keeps
// its scheduler from moving them, wait_vmcnt adds the waits it would not set):
//   kOrderA  rows 0 and 1 as their packets come, row 2 when row 0 is back, row 3 when rows 1 and 2 are; the next step's packets;
//            the compares of rows 0 to 2, and row 3 waited for under those packets.  What the guards of rounds 8 to 14 made the
//            compiler do, and 10 % faster than B while the kernel sat on the fabric (round 10)
//   kOrderB  every row as soon as its packet is there -- four in flight --, the next step's packets, then each row's compares
//            behind a wait for that row alone.  10 % faster than A since round 13 took the kernel off the fabric: kBlockOrder
// (A third order -- the rows of step i + 1 ahead of the compares of step i, in a second set of row registers -- lies between
// the two and is not kept.)  profiles/r15_scan_block_ab.txt has them measured, r15_scan_block_isa.txt their wait sequences.

// s_waitcnt vmcnt(N) and nothing else (gfx9 encoding: vmcnt in bits 3:0 and 15:14; expcnt, bits 6:4, and lgkmcnt, bits 11:8, at
// their maxima, that is not waited for)
template <uint32_t N>
__device__ __forceinline__ void wait_vmcnt()
{
    __builtin_amdgcn_s_waitcnt((N & 15u) | ((N >> 4) << 14) | 0x0f70u);
}

// what a lane holds of a step: NF rows' 16 bytes, and of their packets the pair count and the three pair words
template <int NF>
struct BlockStep {
    uint4 d[NF];
    uint32_t cnt[NF], pr[NF][kPacketPairs];
};

template <int W, int T, int NF = 4, int ORDER = kBlockOrder>
__global__ __launch_bounds__(1024) void scan_block_kernel(const SlabArgs a)
{
    extern __shared__ uint32_t s_cnt[];                                  // [B][T / 4]: a slot's packed counters
    typedef __attribute__((address_space(3))) unsigned long long lds_u64;
    constexpr uint32_t LG = T / 16, NG = 64 / LG, NSUB = kTileBytes / T, NLG = 16 * NG;   // lanes per row piece, pieces per wave-instruction, sub-tiles, lane groups
    constexpr uint32_t STEP = NLG * NF;                                  // packets of a step
    static_assert(LG % 4 == 0, "a lane group is whole quads: each quad loads the packet's four words");
    static_assert(kBlockStepPackets % STEP == 0, "block_list_kernel pads the lists to whole steps");
    static_assert(ORDER != kOrderA || NF == 4, "order A's waits are counted for four packets and rows");
    const uint32_t lane = threadIdx.x & 63u, tid = threadIdx.x;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wg = xcd_workgroup();
    const uint32_t B = a.block_q;
    const uint32_t blk_begin = a.q_begin / B, nblk = (a.q_begin + a.nq - 1) / B - blk_begin + 1;
    if (wg >= a.ntiles * a.r_count * nblk * NSUB) return;               // workgroup-uniform exit
    // item x of the (tile, range): runs of F sub-tiles fastest, then the launch's blocks, then the NSUB / F runs (scalar arithmetic)
    const RangedItem it = ranged_item(a, wg, nblk * NSUB);
    const uint32_t F = a.block_sub_fast, run = it.x / (nblk * F), rem = it.x - run * nblk * F;
    const uint32_t blk = blk_begin + rem / F, sub = run * F + rem % F, r = it.r;
    const uint64_t col0 = (uint64_t)it.tile * kTileBytes + sub * T, row_bytes = (uint64_t)a.G * W;
    if (col0 >= row_bytes) return;                                      // a sub-tile past the last genome: nothing is stored there
    for (uint32_t i = tid; i < B * (T / 16); i += 1024) reinterpret_cast<uint4 *>(s_cnt)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const BlockInfo info = a.binfo[(uint64_t)blk * a.S + r];
    const uint32_t *__restrict__ pkw = reinterpret_cast<const uint32_t *>(a.bpackets + info.base);
    const uint32_t npk = info.npackets, rlo = r * a.range_rows;
    const uint32_t grp = lane / LG, l = lane % LG, lg = wave * NG + grp;
    if (npk) {
        // Lanes whose bytes begin at or past the last genome are given the lane group's FIRST 16 bytes once, here (col0 is below
        // row_bytes, and those bytes are on the line the group fetches anyway): they load and add like the others, into their own
        // cells of the slot's counters, which the epilogue does not store.  The loop knows no dead lanes.
        const uint32_t lcol = col0 + l * 16u < row_bytes ? l * 16u : 0u;
        const uint8_t *__restrict__ hot = a.M + col0 + lcol;
        const uint8_t *__restrict__ cold = cold_home(a.M, a.Mc) + col0 + lcol;
        // the range's home is the workgroup's choice, a scalar one: its rows lie on one side of P_hot (launch_scan_slab)
        const uint8_t *first = (a.P_hot > rlo ? hot : cold) + (uint64_t)rlo * a.ld;
        const uint32_t ld = (uint32_t)a.ld;
        const uint32_t l16 = l * 16u;                                   // the lane's place in a slot's counters
        // A step: NF packets per lane group, a word per lane (each quad of the group has the packet's four).  The list is whole
        // steps (block_list_kernel pads it), so a step's packets are a SCALAR base -- the list's first word plus the step -- and a
        // per-lane byte offset that never changes: no vector arithmetic, no clamp, no test against the list's end.
        const uint32_t pk_lane = (lg * 4u + (lane & 3u)) * 4u;
        uint32_t wd[NF];
        auto load_packets = [&](uint32_t i0) {                          // i0: wave-uniform, a whole step inside the list
            // (a base per 4 KiB, all that a load's immediate offset spans, each kept in SGPRs as row_base keeps a row's: the loads
            // are the saddr form `global_load_dword v, v_lane, s[base] offset:imm`)
            constexpr uint32_t SPAN = 4096;
            // (the empty statement keeps the offset's extension to 64 bits here, beside the loads: hoisted out of the loop it comes
            // back as a register pair, and a vector add per base and step with it)
            uint32_t lane_off = pk_lane;
            asm volatile("" : "+v"(lane_off));
#pragma unroll
            for (uint32_t u = 0; u < (uint32_t)NF; ++u) {
                const uint32_t at = u * NLG * 16u;
                const uint8_t *sp = row_base(reinterpret_cast<const uint8_t *>(pkw) + at / SPAN * SPAN, i0, 16u);
                wd[u] = *reinterpret_cast<const uint32_t *>(sp + at % SPAN + lane_off);
            }
        };
        // the rows of the step whose packets are in wd: the pair count is the header's top byte as it stands (0 in the padding)
        auto request = [&](BlockStep<NF> &s) {
#pragma unroll
            for (uint32_t u = 0; u < (uint32_t)NF; ++u) {
                // ORDER A: row 1 leaves when packets 1 and 2 are there, row 2 when packet 3 and row 0 are, row 3 when rows 1 and 2
                // are -- at most two rows in flight
                if (ORDER == kOrderA) {
                    if (u == 1) wait_vmcnt<2>();
                    if (u == 2) wait_vmcnt<1>();
                    if (u == 3) wait_vmcnt<0>();
                }
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t hdr = quad_word<0>(wd[u]);
                s.pr[u][0] = quad_word<1>(wd[u]); s.pr[u][1] = quad_word<2>(wd[u]); s.pr[u][2] = quad_word<3>(wd[u]);
                s.cnt[u] = hdr >> 24;
                s.d[u] = load_row16<false>(piece_base(first, hdr & 0xffffffu, ld));
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto count = [&](const BlockStep<NF> &s) {
#pragma unroll
            for (uint32_t u = 0; u < (uint32_t)NF; ++u) {
#pragma unroll
                for (uint32_t k = 0; k < kPacketPairs; ++k) {
                    if (k >= s.cnt[u]) continue;
                    // the pair word as the list kernel made it: the broadcast fingerprint is one v_perm_b32, the counters' address
                    // one v_and_or_b32 (W = 1) -- with the four-instruction compare 18 vector instructions per pair block (profiles/r15_scan_block_isa.txt)
                    const uint32_t b = pair_fp<W>(s.pr[u][k]);
                    // (s_cnt is the kernel's only LDS and starts at LDS address 0: the offset IS the address, nothing is added to it)
                    lds_u64 *__restrict__ c2 = reinterpret_cast<lds_u64 *>((uintptr_t)pair_offset<W, T>(s.pr[u][k], l16));
                    // Two no-return ds_add_u64 per pair, two counter words each: no byte (half-word) counter carries -- a (query,
                    // range) has at most 255 (65,535) entries -- so no word carries into the next and the sums are those of four
                    // 32-bit adds.  (A slot's T bytes span T / 4 of the 32 banks, and whatever the slot, lane l of a lane group adds to
                    // banks 4 l ... 4 l + 3: the lane groups of an LDS cycle meet on the same banks.  With four ds_add_u32 that was 8
                    // LDS cycles per add, three quarters of them conflicts, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.747.  Of the
                    // remedies that round 14 probed and built -- profiles/r14_piece_probe.txt, r14_scan_block_ab.txt -- the 64-bit adds
                    // take 1.6 % off the step; slots 33 words apart, which meet only where the slots agree mod 4, probe as well and
                    // LOSE 2 % in the kernel, where they cost forty slots of the block and make a chunk seventeen blocks; a rotated
                    // word order loses in the probe already.  Round 12 had the 64-bit adds 9 % slower: the kernel then waited for
                    // the fabric, r12_scan_block_ab.txt.)
                    __hip_atomic_fetch_add(c2 + 0, (unsigned long long)ne_lanes_block<W>(s.d[u].x, b) | (unsigned long long)ne_lanes_block<W>(s.d[u].y, b) << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(c2 + 1, (unsigned long long)ne_lanes_block<W>(s.d[u].z, b) | (unsigned long long)ne_lanes_block<W>(s.d[u].w, b) << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        };
        load_packets(0);
        // the next step's packets are asked for before this step's rows are used: the rows are waited for under them
        for (uint32_t i0 = 0; i0 < npk; i0 += STEP) {
            BlockStep<NF> s;
            request(s);
            load_packets(i0 + STEP < npk ? i0 + STEP : i0);             // (after the last step: the last step again, a scalar select)
            __builtin_amdgcn_sched_barrier(0);
            count(s);
        }
    }
    __syncthreads();
    const uint32_t qb = blk * B;
    for (uint32_t i = tid; i < B * LG; i += 1024) {
        const uint32_t s = i / LG, piece = i - s * LG, q = qb + s;
        if (q < a.q_begin || q >= a.q_begin + a.nq || col0 + piece * 16u >= row_bytes) continue;
        *reinterpret_cast<uint4 *>(partial_at(a, it.tr, q - a.q_begin) + sub * T + piece * 16u) = reinterpret_cast<const uint4 *>(s_cnt)[i];
    }
}

// ---------------------------------------------------------------- dense queries
// Whole-genome queries (-A) have nearly every partition active: walking a sparse
// list buys nothing and every query would stream the whole matrix on its own.
// Here a wave owns (GB groups of four queries, row tile, chunk of rows): each row piece
// is loaded ONCE and compared against the 4 * GB queries' fingerprints of that
// partition (one scalar dword per group), which divides the bytes per comparison by
// 4 * GB.  Mismatch counters are packed as in the sparse kernel (four byte counters per
// word, spilled every 248 rows into two 16-bit counters per word: the host cuts chunks of
// at most 16,368 rows, dense_chunk_rows, and a 16-bit counter holds 65,535); the wave's
// share of each score is added to the score row with integer atomics (order-independent,
// exact).
template <int W, int GB>
__global__ __launch_bounds__(256) void scan_dense_kernel(const DenseArgs a)
{
    constexpr uint32_t NCNT = 16 / W, FLUSH = W == 1 ? 248u : 65528u, QB = 4 * GB;
    constexpr uint32_t NWORD = 8;                                    // counter words per query (two counters each)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t work = blockIdx.x * 4u + wave;
    const uint32_t nsets = (a.ngroups + GB - 1) / GB;
    if (work >= nsets * a.ntiles * a.nchunks) return;
    const uint32_t chunk = work % a.nchunks, gt = work / a.nchunks;
    const uint32_t tile = gt % a.ntiles, set = gt / a.ntiles;
    if (!RowTile::live<W>(tile, lane, a.G)) return;
    uint32_t qidx[QB];
    bool any = false, grp_on[GB];
#pragma unroll
    for (uint32_t gb = 0; gb < (uint32_t)GB; ++gb) {
        const uint32_t group = set * GB + gb;
        grp_on[gb] = false;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t qi = group < a.ngroups ? a.dense_q[group * 4 + j] : 0xffffffffu;
            qidx[gb * 4 + j] = qi;
            grp_on[gb] |= qi >= a.q0 && qi < a.q1;
        }
        any |= grp_on[gb];
    }
    if (!any) return;
    // this launch walks rows [row_lo, row_hi) (the whole matrix, or one window of it: api_query.hip, scan_windows)
    const uint32_t row0 = a.row_lo + chunk * a.rows_per_item, row1 = min(a.row_hi, row0 + a.rows_per_item);
    const RowTile t = row_tile(a, tile, lane);
    using fp4_t = typename std::conditional<W == 1, uint32_t, uint2>::type;
    const fp4_t *__restrict__ dv[GB];
#pragma unroll
    for (uint32_t gb = 0; gb < (uint32_t)GB; ++gb)
        dv[gb] = reinterpret_cast<const fp4_t *>(a.dense) + (uint64_t)min(set * GB + gb, a.ngroups - 1) * a.P;
    // W == 1: cnt[j][2w] / [2w+1] hold the even / odd byte counters of word w, 16 bits each;
    // W == 2: cnt[j][w] is acc's word w itself (two 16-bit counters), no spill ever needed
    uint32_t cnt[QB][NWORD], nact[QB];
#pragma unroll
    for (uint32_t j = 0; j < QB; ++j) {
        nact[j] = 0;
#pragma unroll
        for (uint32_t k = 0; k < NWORD; ++k) cnt[j][k] = 0;
    }
    for (uint32_t r0 = row0; r0 < row1; r0 += FLUSH) {
        const uint32_t r1 = min(row1, r0 + FLUSH);
        uint4 acc[QB];
#pragma unroll
        for (uint32_t j = 0; j < QB; ++j) acc[j] = make_uint4(0, 0, 0, 0);
        for (uint32_t r = r0; r < r1; r += 4) {
            uint4 d[4];
            fp4_t f[4][GB];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint32_t rr = min(r + u, r1 - 1);                   // tail rows repeat the last (masked below)
#pragma unroll
                for (uint32_t gb = 0; gb < (uint32_t)GB; ++gb) f[u][gb] = dv[gb][rr];
                d[u] = t.load<false>(rr);
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                if (r + u >= r1) break;
#pragma unroll
                for (uint32_t j = 0; j < QB; ++j) {
                    if (!grp_on[j / 4]) continue;                         // wave-uniform
                    const fp4_t &fw = f[u][j / 4];
                    const uint32_t jj = j & 3u;
                    uint32_t fp;
                    if (W == 1) fp = (reinterpret_cast<const uint32_t &>(fw) >> (8 * jj)) & 0xffu;
                    else { const uint2 &ff = reinterpret_cast<const uint2 &>(fw); fp = ((jj < 2 ? ff.x : ff.y) >> (16 * (jj & 1))) & 0xffffu; }
                    if (fp == a.empty) continue;                          // wave-uniform
                    ++nact[j];
                    acc[j] = count_ne<W, false>(acc[j], d[u], bcast_fp<W>(fp));
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < QB; ++j) {
            const uint32_t aw[4] = {acc[j].x, acc[j].y, acc[j].z, acc[j].w};
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                if (W == 1) {
                    cnt[j][2 * w + 0] += aw[w] & 0x00ff00ffu;
                    cnt[j][2 * w + 1] += (aw[w] >> 8) & 0x00ff00ffu;
                } else {
                    cnt[j][w] += aw[w];
                }
            }
        }
    }
    const uint32_t g0 = tile * (kTileBytes / W) + lane * NCNT;
#pragma unroll
    for (uint32_t j = 0; j < QB; ++j) {
        if (qidx[j] < a.q0 || qidx[j] >= a.q1 || nact[j] == 0) continue;
        uint32_t *__restrict__ row = a.scores + (uint64_t)tile * a.score_tile_stride +
                                     (uint64_t)(qidx[j] - a.q0) * a.score_q_stride + lane * NCNT;
#pragma unroll
        for (uint32_t k = 0; k < NCNT; ++k) {
            uint32_t ne;
            if (W == 1) ne = (cnt[j][2 * (k / 4) + (k & 1u)] >> (16 * ((k & 3u) / 2))) & 0xffffu;   // byte k & 3 of word k / 4
            else ne = (cnt[j][k / 2] >> (16 * (k & 1u))) & 0xffffu;
            if (g0 + k < a.G && nact[j] != ne) atomicAdd(row + k, nact[j] - ne);
        }
    }
}

// ---------------------------------------------------------------- dense queries by table (described for one-byte fingerprints;
// two bytes: the last paragraph)
// scan_dense_kernel above tests a row piece against every query on its own -- six vector instructions per four
// comparisons, 48 per data word for its eight queries -- and is bound by exactly those (2.97e13 comparisons/s = 3.85 TB/s x
// 8 queries, half of what HBM would carry).  Here a data word costs about a dozen for EIGHT queries:
//  * "which of the eight queries have this byte at this row" is a function of the byte: mask(v) = T0[v & 3] & T1[(v >> 2) & 3]
//    & T2[(v >> 4) & 3] & T3[v >> 6], where Tf holds, per value of the 2-bit field f, the queries whose fingerprint has that
//    value there (a byte equals a fingerprint iff all four fields do).  The four tables of a row -- four bytes each, made
//    once per set by dense_lut_kernel -- are looked up for the four bytes of a word at once by v_perm_b32 (a four-entry
//    byte table IS one source word, and it comes straight from a scalar register: tables of eight entries need two
//    sources, of which only one may be scalar -- their copies into vector registers cost more than the fourth lookup);
//    the field selectors are shared by every group of eight queries the wave carries.
//  * the masks of successive rows are COUNTED bit by bit: every bit of the mask word (query j of genome byte b) has a
//    counter spread over bit planes, fed by carry-save adders -- sixteen rows go in with fifteen adders of two
//    instructions each (v_bitop3: sum and majority) and one ripple through the upper planes: three instructions per row
//    and word for all eight queries, where the byte counters above took three per query.
// Matches are counted directly (no "active rows minus mismatches"): a query without a fingerprint at a row is in no table.
// Two-byte fingerprints: a fingerprint matches where its low byte matches a query's low byte AND its high byte that query's
// high byte -- two sets of tables per row and octet; a word's high bytes (1 and 3) select from the upper half of an eight-entry
// table (the second source word of v_perm_b32) whose lower half is the low byte's; the byte-wise sets meet by m & (m >> 8).
struct DenseLut { uint32_t t[4]; };   // four 4-entry byte tables, one per 2-bit field of a byte: 16 bytes per (octet of queries, row) at one
                                      // byte per fingerprint; two of them at two bytes (the low byte's tables, then the high byte's)

template <int W>
__global__ __launch_bounds__(256) void dense_lut_kernel(const uint8_t *__restrict__ dense, uint32_t ngroups, uint32_t P, uint32_t empty,
                                                        DenseLut *__restrict__ lut)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x, octet = blockIdx.y;
    if (p >= P) return;
    DenseLut t[2];                                                    // (one byte: the three fields' tables; two bytes: the low byte's, the high byte's)
#pragma unroll
    for (uint32_t x = 0; x < 2u; ++x) t[x].t[0] = t[x].t[1] = t[x].t[2] = t[x].t[3] = 0;
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
        const uint32_t group = octet * 2 + half;
        if (group >= ngroups) break;
        // four queries' fingerprints of this row
        uint32_t f4[W];
        if (W == 1) f4[0] = reinterpret_cast<const uint32_t *>(dense)[(uint64_t)group * P + p];
        else { const uint2 v2 = reinterpret_cast<const uint2 *>(dense)[(uint64_t)group * P + p]; f4[0] = v2.x; f4[W - 1] = v2.y; }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t v = W == 1 ? (f4[0] >> (8 * j)) & 0xffu : (f4[j / 2] >> (16 * (j & 1u))) & 0xffffu, bit = 1u << (half * 4 + j);
            if (v == empty) continue;
            if (W == 1) {
                // fields of three, three and two bits: two eight-entry byte tables (a pair of words each) and a four-entry one
                const uint32_t f0 = v & 7u, f1 = (v >> 3) & 7u, f2 = v >> 6;
                t[0].t[f0 >> 2] |= bit << (8 * (f0 & 3u));
                t[0].t[2 + (f1 >> 2)] |= bit << (8 * (f1 & 3u));
                t[1].t[0] |= bit << (8 * f2);
            } else {
#pragma unroll
                for (uint32_t x = 0; x < 2u; ++x)
#pragma unroll
                    for (uint32_t f = 0; f < 4; ++f) t[x].t[f] |= bit << (8 * ((v >> (8 * x + 2 * f)) & 3u));
            }
        }
    }
#pragma unroll
    for (uint32_t x = 0; x < 2u; ++x) lut[((uint64_t)octet * P + p) * 2 + x] = t[x];
}

// sum and carry of three one-bit inputs per bit position
__device__ __forceinline__ void csa(uint32_t &carry, uint32_t &sum, uint32_t a, uint32_t b, uint32_t c)
{
    carry = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);            // majority: one instruction (v_bitop3_b32)
    sum = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);              // parity: one more
}

// GS: the sets (of NO octets) whose waves SHARE the rows of one (tile, chunk of rows): 1 -- a wave loads its rows itself --, or
// 2 or 4 waves of the workgroup: each loads a share of a batch of eight rows, leaves it in LDS, and all of them work from
// there.  (Round 4 let the sets of a tile walk the same rows as neighbouring waves and trusted the caches: the counters saw
// every row come through the fabric 1.8 times at two sets, and a wave that carries sixteen queries has one neighbour on its
// SIMD to hide a load's latency behind -- vector issue stood at 0.66.)
// (a row's tables are the wave's -- every lane the same address -- and the compiler loads them with VECTOR loads: it cannot know
// that the score rows' atomics do not touch them.  Forced through the constant address space they become scalar loads, and the
// kernel twice as slow at 64 queries (162 against 80 ms: 268 MB of tables stream through a 16 KiB scalar cache): left as it is.)
__device__ __forceinline__ uint4 load_tables16(const DenseLut *p) { return *reinterpret_cast<const uint4 *>(p); }

template <int W, int NO, int GS>
__global__ __launch_bounds__(256) void scan_dense_lut_kernel(const DenseArgs a)
{
    // counts up to 16,383: the host cuts chunks of at most 16,368 rows (dense_chunk_rows)
    constexpr uint32_t kPlanes = 14;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t nsets = (a.noctets + NO - 1) / NO;
    // a sharing group: GS waves, one (tile, chunk) and GS sets; a workgroup holds 4 / GS of them.  A wave without work of its own
    // (a set beyond the last, a group beyond the grid's end, no query of this pass) still loads its share and keeps the barriers
    const uint32_t nsg = (nsets + GS - 1) / GS, ngroups_all = nsg * a.ntiles * a.nchunks;
    const uint32_t grp_in_wg = wave / GS, w_in_grp = wave % GS;
    // Workgroups are dealt to the eight XCDs (xcd_workgroup): XCD x walks the groups x * n / 8 ... in order, and a group's number has
    // the TILE running fastest -- so the workgroups in flight on one XCD walk the same chunk of rows of neighbouring tiles and
    // find that chunk's tables (32 bytes per row and octet, the same for every tile) in their L2 instead of fetching them
    // once per tile (98 x 268 MB at 64 queries: a quarter on top of the matrix at the fabric, profiles/r6_pmc_dense.txt).
    const uint32_t group_id = xcd_workgroup() * (4u / GS) + grp_in_wg;
    const bool group_live = group_id < ngroups_all;
    if (GS == 1 && !group_live) return;
    const uint32_t gid = min(group_id, ngroups_all - 1u);
    const uint32_t tile = gid % a.ntiles, cs = gid / a.ntiles, set = (cs % nsg) * GS + w_in_grp, chunk = cs / nsg;
    const bool lane_live = RowTile::live<W>(tile, lane, a.G);
    // (a lane beyond the tile's last genome stays: it carries its share of the rows' tables, below; its rows lie in the tile's padding)
    uint32_t qidx[NO][8];
    bool any = false;
#pragma unroll
    for (uint32_t o = 0; o < (uint32_t)NO; ++o)
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t slot = (set * NO + o) * 8 + j;
            const uint32_t qi = group_live && set < nsets && slot < a.ngroups * 4 ? a.dense_q[slot] : 0xffffffffu;
            qidx[o][j] = qi;
            any |= qi >= a.q0 && qi < a.q1;
        }
    if (GS == 1 && !any) return;
    const bool working = any && lane_live;                              // (wave-uniform but for the tile's last lanes)
    const uint32_t row0 = a.row_lo + chunk * a.rows_per_item, row1 = min(a.row_hi, row0 + a.rows_per_item);
    const RowTile rows = row_tile(a, tile, lane);
    const DenseLut *__restrict__ lut[NO];
#pragma unroll
    for (uint32_t o = 0; o < (uint32_t)NO; ++o) lut[o] = a.lut + (uint64_t)min(set * NO + o, a.noctets - 1) * a.P * 2;
    // plane[o][w][k]: bit k of the counters of mask word w (bit 8 b + j = query j of octet o against genome byte b of the word).
    // The low EIGHT planes live in registers; a carry out of them -- a counter passes a multiple of 256: at most once per counter in
    // 256 rows -- is OR-ed into a pending word and rippled through the five upper planes, which live in LDS (10 KiB per wave,
    // lane-major: no bank conflicts), once per 256 rows.  (Round 4 rippled every carry of weight sixteen through all nine upper
    // planes, one octet's in registers, the other's in LDS: eighteen instructions per sixteen rows, word and octet; nine now.)
    constexpr uint32_t kRegPlanes = 8, kUp = kPlanes - kRegPlanes;
    __shared__ uint32_t s_up[4][NO * kUp * 4][64];
    uint32_t plane[NO][4][kRegPlanes], pend[NO][4];
#pragma unroll
    for (uint32_t o = 0; o < (uint32_t)NO; ++o)
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            pend[o][w] = 0;
#pragma unroll
            for (uint32_t k = 0; k < kPlanes; ++k) {
                if (k < kRegPlanes) plane[o][w][k] = 0;
                else s_up[wave][(o * kUp + (k - kRegPlanes)) * 4 + w][lane] = 0;
            }
        }
    auto flush_pending = [&]() {                                         // the pending carries of weight 256 into the upper planes
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)NO; ++o)
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                uint32_t c = pend[o][w];
                pend[o][w] = 0;
#pragma unroll
                for (uint32_t k = 0; k < kUp; ++k) {
                    const uint32_t t = s_up[wave][(o * kUp + k) * 4 + w][lane];
                    s_up[wave][(o * kUp + k) * 4 + w][lane] = t ^ c;
                    c &= t;
                }
            }
    };
    constexpr uint32_t RB = GS == 2 ? 4 : 8;                             // rows per batch of loads (two sharing groups in a workgroup: half, for their row buffers' LDS)
    // shared rows: two batches of eight rows (1 KiB each) per sharing group -- one being worked from, one being filled
    constexpr uint32_t kMine = RB / GS;                                  // rows of a batch this wave loads
    __shared__ uint4 s_rows[GS == 1 ? 1 : 4 / GS][GS == 1 ? 1 : 2][GS == 1 ? 1 : RB][GS == 1 ? 1 : 64];
    // (every group of a workgroup makes the same number of passes -- a chunk's rows, clamped at its end -- so that the barriers match)
    const uint32_t row_span = a.rows_per_item;
    auto load_mine = [&](uint32_t rb, uint4 (&v)[kMine]) {               // this wave's share of the batch whose first row is rb
#pragma unroll
        for (uint32_t u = 0; u < kMine; ++u) {
            const uint32_t rr = min(rb + u * GS + w_in_grp, row1 - 1u);
            v[u] = rows.load<false>(rr);
        }
    };
    auto store_mine = [&](uint32_t buf, const uint4 (&v)[kMine]) {
#pragma unroll
        for (uint32_t u = 0; u < kMine; ++u) s_rows[grp_in_wg][buf][u * GS + w_in_grp][lane] = v[u];
    };
    uint32_t nbuf = 0;
    if (GS > 1) {
        uint4 v0[kMine];
        load_mine(row0, v0);
        store_mine(0, v0);
        __syncthreads();
    }
    // The tables of sixteen rows -- 32 bytes per row and octet, 512 bytes per octet: contiguous -- come with ONE load of the wave
    // (a lane: 16 bytes; lanes 0-31 the first octet's, 32-63 the second's, with one octet lanes 32-63 idle along), a block of
    // sixteen rows ahead, and wait in LDS, where a pair of rows' tables are read as broadcasts.  (Before: 68 vector loads of 64
    // equal addresses per sixteen rows and wave -- a third of a wave's cycles were waits for them, profiles/r6_pmc_dense.txt.)
    __shared__ uint4 s_tab[4][2][64];
    auto load_tab = [&](uint32_t rb) {                                   // this lane's piece of the tables of rows [rb, rb + 16)
        const uint32_t o = NO == 2 ? lane >> 5 : 0u, piece = lane & 31u;
        const uint32_t rr = min(rb + (piece >> 1), row1 - 1u);
        return load_tables16(lut[NO == 2 ? o : 0] + (uint64_t)rr * 2 + (piece & 1u));
    };
    uint32_t tbuf = 0;
    uint4 tab_next = load_tab(row0);
    for (uint32_t r = row0; r < (GS == 1 ? row1 : row0 + row_span); r += 16) {
        uint32_t twosP[NO][4], foursP[NO][4], eightsP[NO][4];            // carries waiting for their partner
        s_tab[wave][tbuf][lane] = tab_next;                              // (this block's tables: in LDS before its first pair asks)
        tab_next = load_tab(r + 16);
#pragma unroll
        for (uint32_t bt = 0; bt < 16 / RB; ++bt) {                       // a batch: its loads first (all in flight), then the work
            uint4 d[RB];
            uint4 vnext[kMine];
            if (GS == 1) {
#pragma unroll
                for (uint32_t u = 0; u < RB; ++u) d[u] = rows.load<false>(r + bt * RB + u);
            } else {
                // the NEXT batch's share from memory (in flight under this batch's work), this batch's rows from LDS
                load_mine(r + bt * RB + RB, vnext);
#pragma unroll
                for (uint32_t u = 0; u < RB; ++u) d[u] = s_rows[grp_in_wg][nbuf][u][lane];
            }
            if (GS == 1 || (working && r < row1)) {
            // Two rows at a time (their tables: four scalar words per row and octet, asked for when their turn comes -- all
            // rows' tables at once do not fit the scalar registers and end up as vector copies): masks of the pair's four words,
            // into the ones; a carry waits for its partner of the same weight.  The fences keep the compiler from pooling the pairs.
#pragma unroll
            for (uint32_t pp = 0; pp < RB / 2; ++pp) {
                const uint32_t pr = bt * (RB / 2) + pp;                   // pair 0 .. 7 of the sixteen rows
                __builtin_amdgcn_sched_barrier(0);
                // this pair's tables: four (eight) broadcast reads
                uint4 tb[2][NO][2];
#pragma unroll
                for (uint32_t v = 0; v < 2; ++v)
#pragma unroll
                    for (uint32_t o = 0; o < (uint32_t)NO; ++o)
#pragma unroll
                        for (uint32_t x = 0; x < 2u; ++x) tb[v][o][x] = s_tab[wave][tbuf][o * 32u + (pr * 2u + v) * 2u + x];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (uint32_t w = 0; w < 4; ++w) {
                    uint32_t sel[2][4];
#pragma unroll
                    for (uint32_t v = 0; v < 2; ++v) {
                        const uint4 &dd = d[pp * 2 + v];
                        const uint32_t dw = w == 0 ? dd.x : w == 1 ? dd.y : w == 2 ? dd.z : dd.w;
                        if (W == 1) { sel[v][0] = dw & 0x07070707u; sel[v][1] = (dw >> 3) & 0x07070707u; sel[v][2] = (dw >> 6) & 0x03030303u; sel[v][3] = 0; }
                        else { sel[v][0] = dw & 0x03030303u; sel[v][1] = (dw >> 2) & 0x03030303u; sel[v][2] = (dw >> 4) & 0x03030303u; sel[v][3] = (dw >> 6) & 0x03030303u; }
                        // two-byte fingerprints: a word's high bytes (1 and 3) look their fields up in the high byte's tables -- the
                        // upper half of an eight-entry table whose lower half is the low byte's
                        if (W == 2) { sel[v][0] |= 0x04000400u; sel[v][1] |= 0x04000400u; sel[v][2] |= 0x04000400u; sel[v][3] |= 0x04000400u; }
                    }
#pragma unroll
                    for (uint32_t o = 0; o < (uint32_t)NO; ++o) {
                        uint32_t m[2];
#pragma unroll
                        for (uint32_t v = 0; v < 2; ++v) {
                            const uint4 lo = tb[v][o][0], hi = tb[v][o][1];
                            if (W == 1) {
                                // three lookups -- two in eight-entry tables (a pair of words: v_perm_b32's two sources, of which the
                                // compiler copies one into a vector register per row: a quarter of an instruction per word) and one in
                                // a four-entry table -- and ONE three-input AND
                                m[v] = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_perm(lo.y, lo.x, sel[v][0]), __builtin_amdgcn_perm(lo.w, lo.z, sel[v][1]),
                                                                   __builtin_amdgcn_perm(0u, hi.x, sel[v][2]), 0x80);
                            } else {
                                const uint32_t both = __builtin_amdgcn_perm(hi.x, lo.x, sel[v][0]) & __builtin_amdgcn_perm(hi.y, lo.y, sel[v][1]) &
                                                      __builtin_amdgcn_perm(hi.z, lo.z, sel[v][2]) & __builtin_amdgcn_perm(hi.w, lo.w, sel[v][3]);
                                // (two bytes: a fingerprint matches where its low byte's set and its high byte's meet; the result sits in the low byte's place)
                                m[v] = both & (both >> 8) & 0x00ff00ffu;
                            }
                        }
                        uint32_t twos;
                        csa(twos, plane[o][w][0], plane[o][w][0], m[0], m[1]);
                        if (!(pr & 1u)) { twosP[o][w] = twos; continue; }
                        uint32_t fours;
                        csa(fours, plane[o][w][1], plane[o][w][1], twosP[o][w], twos);
                        if (!(pr & 2u)) { foursP[o][w] = fours; continue; }
                        uint32_t eights;
                        csa(eights, plane[o][w][2], plane[o][w][2], foursP[o][w], fours);
                        if (!(pr & 4u)) { eightsP[o][w] = eights; continue; }
                        uint32_t carry;
                        csa(carry, plane[o][w][3], plane[o][w][3], eightsP[o][w], eights);
                        // one bit of weight sixteen per position: through planes 4-7, what falls out of them waits in `pend`
#pragma unroll
                        for (uint32_t k = 4; k < kRegPlanes; ++k) {
                            const uint32_t t = plane[o][w][k];
                            plane[o][w][k] = t ^ carry;
                            carry &= t;
                        }
                        pend[o][w] |= carry;
                    }
                }
            }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (GS > 1) {                                                 // the next batch into the other half; everybody has read this one after the barrier
                store_mine(nbuf ^ 1u, vnext);
                nbuf ^= 1u;
                __syncthreads();
            }
        }
        tbuf ^= 1u;
        if ((((r - row0) >> 4) & 15u) == 15u) flush_pending();            // (256 rows since the last time: wave-uniform)
    }
    if (!working) return;
    flush_pending();
    // the counters' planes -> numbers, query by query: four genomes of a word at a time (low eight planes into byte counters,
    // the upper planes into a second set), added to the score rows with integer atomics
#pragma unroll
    for (uint32_t o = 0; o < (uint32_t)NO; ++o)
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t qi = qidx[o][j];
            if (qi < a.q0 || qi >= a.q1) continue;                       // wave-uniform
            constexpr uint32_t NCNT = 16 / W;                             // genomes per lane
            uint32_t *__restrict__ row = a.scores + (uint64_t)tile * a.score_tile_stride + (uint64_t)(qi - a.q0) * a.score_q_stride + lane * NCNT;
            const uint32_t g0 = tile * (kTileBytes / W) + lane * NCNT;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) {
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    const uint32_t pl = plane[o][w][k];
                    lo += ((pl >> j) & 0x01010101u) << k;
                }
#pragma unroll
                for (uint32_t k = 8; k < kPlanes; ++k) {                   // (at most six planes: the upper count stays below 64)
                    const uint32_t pl = s_up[wave][(o * kUp + (k - kRegPlanes)) * 4 + w][lane];
                    hi += ((pl >> j) & 0x01010101u) << (k - 8);
                }
#pragma unroll
                for (uint32_t b = 0; b < 4; b += W) {                      // (two bytes: the counts sit in bytes 0 and 2 of the word)
                    const uint32_t n = ((lo >> (8 * b)) & 0xffu) | (((hi >> (8 * b)) & 0xffu) << 8);
                    const uint32_t gi = (w * 4 + b) / W;
                    if (n && g0 + gi < a.G) atomicAdd(row + gi, n);
                }
            }
        }
}

}  // namespace mk
