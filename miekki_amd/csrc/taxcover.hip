// K6h: distinct covered cells per node of a taxonomy -- per node, how many distinct (partition, value) cells its genomes hold
// and how many of those the sample has seen (mk_taxonomy_cover).
//
//   H(n, p)     { column_g[p] : lo[n] <= g < hi[n], column_g[p] != empty }
//   held(n)     sum over p of |H(n, p)|
//   covered(n)  sum over p of |{ v in H(n, p) : seen(p, v) }|
//
// A node is an interval of genome ids and a row is contiguous in genome id, so a node owns ONE BYTE SEGMENT of every row:
// nothing has to be ordered between genomes, and a row's answer is the number of distinct values in its segment.  A work item
// is (node, chunk of rows); the host lists the items of the nodes of width >= 2 (a node of one genome has held = sketch_size
// and covered = the plain count's) with about kItemBytes of matrix each.  Per item and row the values met are a SET in LDS:
//   one byte:   256 bits.  `sub` lanes of a wave take a row -- 64 (WIDE: the wave strides the segment piece by piece, the next
//               piece in flight) or, for a NARROW node of a few 16-byte pieces, the power of two from 8 on that covers them,
//               so that a wave has 64 / sub rows in hand at once, a 32-byte set each.  A lane ORs its values in behind a plain
//               read (the bits only grow within a row: a stale 0 costs an atomic); then eight lanes take a word each:
//               popcount(set) and popcount(set & the row's slice of seen), and the word is cleared.  `empty` is never put in.
//   two bytes:  8 KiB per wave, four sets per workgroup.  The fetch-or returns the old word: a bit that was newly set adds 1 to
//               held and, when seen(p, v) -- looked up where the table lies, a piece's eight lookups in flight together -- 1 to
//               covered.  Before the next row a NARROW node clears the words its values touched -- from the registers when the
//               segment is a piece per lane, a wider one by a second walk of the row -- and a WIDE node the whole set.  (A
//               workgroup per item with one set for the widest nodes was measured and left out: a barrier and 256 lanes'
//               clearing per row made the root 2.3 times slower than the wave, profiles/taxon_cover.txt.)
// Segments start and end at any genome: aligned 16-byte pieces are loaded and masked to lo <= g < hi (hi <= G: columns
// [G, pitch) are padding and never counted).  A lane counts in 32 bits over an item's rows (at most kMaxRows of them: a lane
// adds at most 65,535 per row); one wave reduction and one relaxed agent-scope 64-bit add per counter (and wave) end the item.
// The pass reads sum over the nodes of width >= 2 of width x P x W bytes: one read of the matrix per level of the taxonomy,
// cold rows where they lie (mat_row), once per level over PCIe.
#include <algorithm>
#include <cerrno>
#include <cstdlib>

#include "mk_internal.hpp"

namespace mk {

namespace {

constexpr uint32_t kMaxRows = 32768;      // rows of an item: 32768 x 65535 < 2^32, a lane's count cannot wrap
constexpr uint64_t kItemBytes = 65536;    // bytes of the matrix an item aims at

__device__ __forceinline__ uint32_t set_load(const uint32_t *w) { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void set_store(uint32_t *w, uint32_t x) { __hip_atomic_store(w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// both counters of an item: a wave's sum, one add each
__device__ __forceinline__ void item_flush(uint32_t held, uint32_t cov, uint32_t lane, mk_node_cover *__restrict__ o)
{
    uint64_t h = held, c = cov;
#pragma unroll
    for (uint32_t s = 32; s > 0; s >>= 1) {
        h += __shfl_xor(h, s);
        c += __shfl_xor(c, s);
    }
    if (lane == 0) {
        if (h) (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(&o->held), (unsigned long long)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c) (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(&o->covered), (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one byte: a wave per item, `sub` lanes per row
__global__ __launch_bounds__(256) void taxcover1_kernel(MatRef M, uint64_t ld, const TaxItem *__restrict__ items, uint32_t n_items,
                                                        const uint32_t *__restrict__ lo_of, const uint32_t *__restrict__ hi_of,
                                                        const uint32_t *__restrict__ seen, mk_node_cover *__restrict__ out)
{
    __shared__ uint32_t s_set[4][64];                                      // a wave's sets: 64 / sub of 8 words
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * 4u + wave;
    if (i >= n_items) return;                                              // (wave-uniform; no workgroup barrier below)
    const TaxItem it = items[i];
    const uint32_t lo = lo_of[it.node], hi = hi_of[it.node];
    const uint32_t sub = it.sub, nsub = 64u / sub, sg = lane / sub, sl = lane & (sub - 1u);
    uint32_t *set = s_set[wave] + sg * 8u;
    s_set[wave][lane] = 0;
    wave_sync();
    const uint64_t b_lo = (uint64_t)(lo & ~15u) + sl * 16u, step = sub * 16u;      // this lane's first piece of a row; b_lo < hi: it has one
    const bool mine = b_lo < hi;
    uint32_t held = 0, cov = 0;
    uint4 nxt = make_uint4(0, 0, 0, 0);
    if (mine && it.r_lo + sg < it.r_hi) nxt = *reinterpret_cast<const uint4 *>(mat_row(M, it.r_lo + sg, ld) + b_lo);
    for (uint32_t r0 = it.r_lo; r0 < it.r_hi; r0 += nsub) {               // (uniform: the barriers are the whole wave's)
        const uint32_t r = r0 + sg;
        const bool active = r < it.r_hi;
        if (active && mine) {
            const uint8_t *row = mat_row(M, r, ld);
            for (uint64_t b = b_lo; b < hi; b += step) {
                const uint4 cur = nxt;
                // the next piece in flight: of this row, or the first of this lane's next row
                if (b + step < hi) nxt = *reinterpret_cast<const uint4 *>(row + b + step);
                else if (r + nsub < it.r_hi) nxt = *reinterpret_cast<const uint4 *>(mat_row(M, r + nsub, ld) + b_lo);
                const uint32_t x[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                for (uint32_t j = 0; j < 16; ++j) {
                    const uint32_t v = (x[j / 4] >> ((j * 8u) & 31u)) & 255u;
                    const uint64_t g = b + j;
                    if (g < lo || g >= hi || v == 255u) continue;          // another node's, padding (hi <= G), `empty`
                    uint32_t *w = set + (v >> 5);
                    const uint32_t m = 1u << (v & 31u);
                    if (!(set_load(w) & m)) (void)__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        wave_sync();
        if (active && sl < 8u) {
            const uint32_t w = set_load(set + sl);
            uint32_t s = seen ? seen[(uint64_t)r * 8u + sl] : 0u;
            if (sl == 7u) s &= 0x7fffffffu;                                // the slice's last bit is `empty`'s
            held += __popc(w);
            cov += __popc(w & s);
            set_store(set + sl, 0u);
        }
        wave_sync();
    }
    item_flush(held, cov, lane, out + it.node);
}

// two bytes: a wave per item with a set of its own; sub = 64: the whole set is cleared between rows, any other: the touched words
__global__ __launch_bounds__(256) void taxcover2_kernel(MatRef M, uint64_t ld, const TaxItem *__restrict__ items, uint32_t n_items,
                                                        const uint32_t *__restrict__ lo_of, const uint32_t *__restrict__ hi_of,
                                                        const uint32_t *__restrict__ seen, mk_node_cover *__restrict__ out)
{
    constexpr uint32_t kWords = 2048u;
    constexpr uint64_t kStep = 64u * 16u;                                  // bytes of a row the wave takes at a time
    __shared__ uint32_t s_set[4][kWords];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * 4u + wave;
    if (i >= n_items) return;                                              // (wave-uniform; no workgroup barrier below)
    const TaxItem it = items[i];
    const uint32_t lo = lo_of[it.node], hi = hi_of[it.node];
    const bool whole = it.sub == 64u;
    uint32_t *set = s_set[wave];
    for (uint32_t s = lane; s < kWords; s += 64u) set[s] = 0;
    wave_sync();
    const uint64_t b_end = (uint64_t)hi * 2u, b_lo = (((uint64_t)lo * 2u) & ~15ull) + lane * 16u;   // the segment's bytes, this lane's first piece
    uint32_t held = 0, cov = 0;
    // the value of slot j of a piece at byte b, 65535 (`empty`: nothing to do) for another node's and for padding (hi <= G)
    auto value = [&](const uint4 &p, uint64_t b, uint32_t j) {
        const uint32_t x[4] = {p.x, p.y, p.z, p.w};
        const uint32_t v = (x[j / 2] >> ((j * 16u) & 31u)) & 65535u;
        const uint64_t g = (b >> 1) + j;
        return g >= lo && g < hi ? v : 65535u;
    };
    uint4 nxt = make_uint4(0, 0, 0, 0), first = nxt;
    if (b_lo < b_end) nxt = *reinterpret_cast<const uint4 *>(mat_row(M, it.r_lo, ld) + b_lo);
    for (uint32_t r = it.r_lo; r < it.r_hi; ++r) {
        const uint8_t *row = mat_row(M, r, ld);
        const uint32_t *sl = seen ? seen + (uint64_t)r * kWords : nullptr; // the row's 8 KiB slice, looked up where it lies
        for (uint64_t b = b_lo; b < b_end; b += kStep) {
            const uint4 cur = nxt;
            if (b == b_lo) first = cur;
            // the next piece in flight: of this row, or the first of the next row
            if (b + kStep < b_end) nxt = *reinterpret_cast<const uint4 *>(row + b + kStep);
            else if (r + 1 < it.r_hi) nxt = *reinterpret_cast<const uint4 *>(mat_row(M, r + 1, ld) + b_lo);
            // into the set: a bit that was newly set counts ...
            uint32_t fresh = 0;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t v = value(cur, b, j);
                if (v == 65535u) continue;
                uint32_t *w = set + (v >> 5);
                const uint32_t m = 1u << (v & 31u);
                if (set_load(w) & m) continue;                             // (the bits only grow within a row: a 1 is not stale)
                if (!(__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & m)) fresh |= 1u << j;
            }
            held += __popc(fresh);
            // ... and is looked up: the eight loads go out together (a slot that is not fresh reads word 0 and counts nothing)
            if (sl && fresh) {
                uint32_t w[8];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) w[j] = sl[(fresh >> j) & 1u ? value(cur, b, j) >> 5 : 0u];
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) cov += (fresh >> j) & (w[j] >> (value(cur, b, j) & 31u)) & 1u;
            }
        }
        wave_sync();
        if (whole) {
            for (uint32_t s = lane; s < kWords; s += 64u) set[s] = 0;
        } else {
            // the words this lane's values touched: the first piece from its register, any other read again
            for (uint64_t b = b_lo; b < b_end; b += kStep) {
                const uint4 p = b == b_lo ? first : *reinterpret_cast<const uint4 *>(row + b);
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) {
                    const uint32_t v = value(p, b, j);
                    if (v != 65535u) set_store(set + (v >> 5), 0u);
                }
            }
        }
        wave_sync();
    }
    item_flush(held, cov, lane, out + it.node);
}

// a switch that takes a whole number from `least` on; absent: *value stays
int read_switch(const char *name, long least, long *value)
{
    const char *e = getenv(name);
    if (!e) return MK_OK;
    char *end = nullptr;
    errno = 0;
    const long v = strtol(e, &end, 10);
    if (errno || end == e || *end || v < least) {
        set_error("%s takes a whole number from %ld on: '%s'", name, least, e);
        return MK_ERR_ARG;
    }
    *value = v;
    return MK_OK;
}

}  // namespace

// MIEKKI_TAXCOVER_ROWS: rows per item for every node (0: by the node's width); MIEKKI_TAXCOVER_WIDE: the width in genomes from
// which a node takes the wide path -- 512 at both widths: 32 pieces at one byte (a narrower node leaves room for two rows and
// more per wave), 64 at two (a piece per lane: the values stay in registers).  The tests send small indexes down every path
// with them.
int taxcover_switches(const mk_ctx *c, uint32_t *rows, uint32_t *wide)
{
    (void)c;
    long r = 0, w = 512;
    MK_TRY(read_switch("MIEKKI_TAXCOVER_ROWS", 1, &r));
    MK_TRY(read_switch("MIEKKI_TAXCOVER_WIDE", 2, &w));
    if (rows) *rows = (uint32_t)std::min<long>(r, kMaxRows);
    if (wide) *wide = (uint32_t)std::min<long>(w, 0x7fffffffL);
    return MK_OK;
}

// The items of the nodes of width >= 2, in node order, a wave each.  Rows per item: about kItemBytes of the node's segments,
// kMaxRows at the most.  sub: 64 for a wide node; for a narrow one the lanes that take a row at one byte, 0 at two.
int taxcover_items(const mk_ctx *c, const uint32_t *lo, const uint32_t *hi, uint32_t n_nodes, uint32_t rows_switch, uint32_t wide,
                   std::vector<TaxItem> &items)
{
    const uint32_t P = c->P, W = c->W;
    for (uint32_t n = 0; n < n_nodes; ++n) {
        const uint64_t width = (uint64_t)hi[n] - lo[n];
        if (width < 2) continue;
        uint32_t sub = 64;
        if (width < wide) {
            const uint64_t pieces = ((uint64_t)hi[n] + 15) / 16 - lo[n] / 16;
            if (W == 1) for (sub = 8; sub < 64 && sub < pieces; sub *= 2) {}
            else sub = 0;
        }
        uint64_t rows = rows_switch ? rows_switch : std::max<uint64_t>(1, kItemBytes / (width * W));
        if (!rows_switch && W == 1) rows = std::max<uint64_t>(rows, 64u / sub);   // (a row for every group of lanes)
        rows = std::min<uint64_t>(std::min<uint64_t>(rows, kMaxRows), P);
        for (uint64_t r = 0; r < P; r += rows) items.push_back(TaxItem{n, (uint32_t)r, (uint32_t)std::min<uint64_t>(P, r + rows), sub});
    }
    if (items.size() > 0x7fffffffull) { set_error("the taxonomy's nodes make more than 2^31 work items"); return MK_ERR_ARG; }
    return MK_OK;
}

// d_out[node] is ADDED to: the caller zeroes it.  d_seen may be null: nothing is covered.  Raw cold rows.
int launch_taxcover(mk_ctx *c, const TaxItem *d_items, uint32_t n_items, const uint32_t *d_lo, const uint32_t *d_hi, const uint32_t *d_seen,
                    mk_node_cover *d_out)
{
    if (!n_items) return MK_OK;
    const dim3 grid((n_items + 3) / 4), block(256);
    if (c->W == 1) hipLaunchKernelGGL(taxcover1_kernel, grid, block, 0, c->stream, mat_ref(c), c->ld, d_items, n_items, d_lo, d_hi, d_seen, d_out);
    else hipLaunchKernelGGL(taxcover2_kernel, grid, block, 0, c->stream, mat_ref(c), c->ld, d_items, n_items, d_lo, d_hi, d_seen, d_out);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
