// K6g: breadth of coverage -- per indexed genome, how many of its stored fingerprints turn up anywhere in a set of queries.
//
//   seen(p, v)   some query of the set has the GATED sketch value v != empty at partition p (minhash_sketch_partition_solid_kmers,
//                Miekki.cpp:214-224: the sketch query_sequence scores with)
//   covered(g)   #{ p : column_g[p] != empty and seen(p, column_g[p]) }
//   cells        #{ (p, v) : seen(p, v) }
//
// `seen` is a table of one bit per (partition, fingerprint value) in caller-owned device memory: bit ((p << fp_bits) + v) & 31
// of 32-bit word ((p << fp_bits) + v) >> 5, P << fp_bits >> 3 bytes.  One-byte fingerprints have a noise floor: an unrelated
// genome is covered at about cells / (P * 256) of its sketch by chance, which is why `cells` is reported next to the counts.
//
//   mark:   the set's gated sketch OR-ed into the table by table_pass.hpp's walks.  Waves on every XCD OR into the same words
//           and the per-XCD L2s are not coherent, so -- as for tally.hip's counters -- every mark is an agent-scope atomic;
//           relaxed, because nothing reads the table inside the pass and the result of the OR is not used; later launches and
//           copies on the stream see it.
//           FILTER: a plain load in front of the atomic, which is skipped when the bit already reads 1.  A stale 0 costs an
//           atomic; a 1 cannot be stale, bits are never cleared inside a pass.
//   count:  table_pass.hpp's pass with a bit for a cell, staged at both widths: the slices of 256 rows at one byte per
//           fingerprint (32 B each), the slice of one row at two (8 KiB).  A lane looks each of its fingerprints up with one
//           LDS dword read (one byte: a wave's reads fall on the 8 dwords of one slice, which broadcast; two bytes: random
//           dwords of 2,048).  At the end of the chunk: one relaxed agent-scope add per genome with a count.
//   cells:  a popcount reduction of the table.
//   win:    the winner-takes-all pass (mk_cover_assign): every seen cell that some genome holds is credited to ONE holder, the
//           one of smallest rank in a caller-given order, and won(g) counts the cells g wins.  Per row an LDS table of one u32
//           per fingerprint value, 0 = nobody; every live, seen genome g < G does an LDS atomic max of G - rank(g) into its
//           value's slot behind a plain LDS read (FILTER: the slot only grows, so a stale read costs an atomic and never a
//           wrong answer).  Once the row is through, every non-zero slot names its winner: one relaxed agent-scope add of 1 to
//           won[order[G - slot]] (the read-out, not a second walk of the row), and the slot is cleared.
//           One byte: a wave per row with a 1 KiB table of its own and the row's 32-byte slice of `seen` in LDS (the bit of
//           `empty` cleared on the way in); a workgroup takes a chunk of rows, the next tile's load is in flight; no
//           workgroup barrier.  Two bytes: a workgroup per row, the values cut into ranges of V slots that fit LDS (16,384 by
//           default: 64 KiB, two workgroups per CU); a row passes once per range, from L2 after the first, a cold row over PCIe
//           each time.  The first lane to raise a slot from 0 appends it to a list of touched slots, and the read-out walks
//           the list; a list that overflows (2,048 slots), or MIEKKI_WIN_TOUCHED=0, reads the whole range out.
#include <algorithm>
#include <cstdlib>

#include "table_pass.hpp"

namespace mk {

namespace {

template <bool FILTER>
__device__ __forceinline__ void mark(uint32_t *__restrict__ seen, uint64_t bit)
{
    uint32_t *w = seen + (bit >> 5);
    const uint32_t m = 1u << ((uint32_t)bit & 31u);
    if (FILTER && (*w & m)) return;
    (void)__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the table of bits as the pass reads it (table_pass.hpp)
struct BitTable {
    using Cell = uint32_t;
    static constexpr uint32_t kCellBits = 1;
    static __device__ __forceinline__ void clear_empty(uint4 &last) { last.w &= 0x7fffffffu; }   // the slice's last bit is `empty`'s
    static __device__ __forceinline__ uint32_t lookup(const uint32_t *sl, uint32_t v) { return (sl[v >> 5] >> (v & 31u)) & 1u; }
};

// covered[g] += the bits a genome's fingerprints find set
struct CoverCount {
    uint32_t *covered;
    __device__ __forceinline__ uint32_t start(uint32_t, uint32_t) const { return 0u; }
    static __device__ __forceinline__ void add(uint32_t &cnt, uint32_t &, uint32_t m) { cnt += m; }
    __device__ __forceinline__ void flush(uint32_t cnt, uint32_t, uint32_t g0, uint32_t j) const
    {
        (void)__hip_atomic_fetch_add(covered + g0 + j, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ __launch_bounds__(256) void cover_cells_kernel(const uint4 *__restrict__ seen4, uint64_t nvec, unsigned long long *__restrict__ cells)
{
    uint32_t n = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nvec; i += (uint64_t)gridDim.x * 256u) {
        const uint4 x = seen4[i];
        n += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);          // (a lane's share stays far below 2^32: at most 2^44 bits over >= 256 lanes)
    }
    uint64_t total = n;
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    if ((threadIdx.x & 63u) == 0 && total) (void)__hip_atomic_fetch_add(cells, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// slot = max(slot, key) behind a plain read (filter; uniform); returns true when this lane raised the slot from 0
constexpr uint32_t kWinTouched = 1u, kWinNoFilter = 2u;                    // the kernels' `flags`
__device__ __forceinline__ bool win_raise(uint32_t *slot, uint32_t key, uint32_t flags)
{
    if (!(flags & kWinNoFilter) && __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= key) return false;
    return __hip_atomic_fetch_max(slot, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0;
}

// a non-zero slot names its winner, order[G - slot], which gets the cell; the slot is cleared for the next row
__device__ __forceinline__ void win_credit(uint32_t *slot, uint32_t G, const uint32_t *__restrict__ order, uint32_t *__restrict__ won)
{
    const uint32_t key = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (!key) return;
    (void)__hip_atomic_fetch_add(won + order[G - key], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

constexpr uint32_t kWinList = 2048;       // touched slots a row's range may list before the whole range is read out (two bytes)

template <int W> __global__ void cover_win_kernel(MatRef, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t *);

// one byte: a wave per row, 256 slots and the row's slice of `seen` of its own (values and kWinTouched are not used)
template <>
__global__ __launch_bounds__(256) void cover_win_kernel<1>(MatRef M, uint64_t ld, uint32_t P, uint32_t G, uint32_t ntiles, uint32_t rows_per_chunk,
                                                           uint32_t values, uint32_t flags, const uint32_t *__restrict__ seen,
                                                           const uint32_t *__restrict__ rank, const uint32_t *__restrict__ order, uint32_t *__restrict__ won)
{
    __shared__ uint32_t s_tab[4][256];
    __shared__ uint32_t s_seen[4][8];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t r_lo = blockIdx.x * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);          // (rows_per_chunk <= P <= 2^28)
    uint32_t *tab = s_tab[wave], *sl = s_seen[wave];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) tab[lane + 64u * k] = 0;
    for (uint32_t r = r_lo + wave; r < r_hi; r += 4u) {
        uint32_t w = lane < 8u ? seen[(uint64_t)r * 8u + lane] : 0u;
        if (lane == 7u) w &= 0x7fffffffu;                                  // the slice's last bit is `empty`'s
        if (!__ballot(w != 0u)) continue;                                  // (uniform: nothing of this row is seen)
        if (lane < 8u) sl[lane] = w;
        wave_sync();
        const uint8_t *row = mat_row(M, r, ld) + lane * 16u;
        uint4 cur = *reinterpret_cast<const uint4 *>(row), nxt = cur;
        for (uint32_t t = 0; t < ntiles; ++t) {
            if (t + 1 < ntiles) nxt = *reinterpret_cast<const uint4 *>(row + (uint64_t)(t + 1) * kTileBytes);
            const uint32_t x[4] = {cur.x, cur.y, cur.z, cur.w};
            const uint32_t g0 = t * kTileBytes + lane * 16u;
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t v = (x[j / 4] >> ((j * 8u) & 31u)) & 255u, g = g0 + j;
                if (g < G && ((sl[v >> 5] >> (v & 31u)) & 1u)) (void)win_raise(tab + v, G - rank[g], flags);   // (columns [G, pitch) are padding)
            }
            cur = nxt;
        }
        wave_sync();
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) win_credit(tab + lane + 64u * k, G, order, won);
        wave_sync();
    }
}

// two bytes: a workgroup per row, the values in ranges of `values` slots: s_dyn = [slots: values][list: kWinList][listed: 1]
template <>
__global__ __launch_bounds__(256) void cover_win_kernel<2>(MatRef M, uint64_t ld, uint32_t P, uint32_t G, uint32_t ntiles, uint32_t rows_per_chunk,
                                                           uint32_t values, uint32_t flags, const uint32_t *__restrict__ seen,
                                                           const uint32_t *__restrict__ rank, const uint32_t *__restrict__ order, uint32_t *__restrict__ won)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    uint32_t *tab = s_dyn, *list = s_dyn + values, *listed = list + kWinList;
    const uint32_t tid = threadIdx.x, touched = flags & kWinTouched;
    const uint32_t r_lo = blockIdx.x * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);
    const uint32_t nvec = ntiles * (kTileBytes / 16u);                     // uint4s of a row: whole tiles, which ld covers
    for (uint32_t s = tid; s < values; s += 256u) tab[s] = 0;
    if (tid == 0) *listed = 0;
    __syncthreads();
    for (uint32_t r = r_lo; r < r_hi; ++r) {
        const uint4 *row = reinterpret_cast<const uint4 *>(mat_row(M, r, ld));
        const uint32_t *sl = seen + (uint64_t)r * 2048u;                   // the row's 8 KiB slice, looked up where it lies
        for (uint32_t v0 = 0; v0 < 65536u; v0 += values) {
            uint4 cur = tid < nvec ? row[tid] : make_uint4(0, 0, 0, 0), nxt = cur;
            for (uint32_t i = tid; i < nvec; i += 256u) {
                if (i + 256u < nvec) nxt = row[i + 256u];
                const uint32_t x[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) {
                    const uint32_t v = (x[j / 2] >> ((j * 16u) & 31u)) & 65535u, g = i * 8u + j;
                    if (g >= G || v == 65535u || v - v0 >= values) continue;          // padding, `empty`, another range's (unsigned)
                    if (!((sl[v >> 5] >> (v & 31u)) & 1u)) continue;
                    if (win_raise(tab + (v - v0), G - rank[g], flags) && touched) {
                        const uint32_t at = __hip_atomic_fetch_add(listed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (at < kWinList) list[at] = v - v0;
                    }
                }
                cur = nxt;
            }
            __syncthreads();
            const uint32_t n = *listed;
            __syncthreads();
            if (tid == 0) *listed = 0;
            if (touched && n <= kWinList) {
                for (uint32_t i = tid; i < n; i += 256u) win_credit(tab + list[i], G, order, won);
            } else {
                for (uint32_t s = tid; s < values; s += 256u) win_credit(tab + s, G, order, won);
            }
            __syncthreads();
        }
    }
}

}  // namespace

uint64_t cover_table_bytes(const mk_ctx *c) { return ((uint64_t)c->P << c->p.fp_bits) >> 3; }

int launch_cover_reset(mk_ctx *c, uint32_t *d_seen)
{
    MK_HIP(hipMemsetAsync(d_seen, 0, cover_table_bytes(c), c->stream));
    return MK_OK;
}

// MIEKKI_COVER_FILTER=0 / 1: the marks without / with the plain load in front of the atomic (tools/cover_rate.py measures both)
static bool cover_filter()
{
    if (const char *e = getenv("MIEKKI_COVER_FILTER")) return atol(e) != 0;
    return true;
}

int launch_cover_mark(mk_ctx *c, const mk_qset *qs, uint32_t *d_seen)
{
    return launch_table_mark<uint32_t, mark<false>, mark<true>>(c, qs, cover_filter(), d_seen);
}

// d_covered[G] and *d_cells are ADDED to: the caller zeroes them
int launch_cover_count(mk_ctx *c, const uint32_t *d_seen, uint32_t *d_covered, unsigned long long *d_cells)
{
    if (d_covered && c->G) {
        PassGrid g;
        MK_TRY(table_pass_grid<BitTable>(c, "MIEKKI_COVER_ROWS", &g));
        launch_table_pass<BitTable>(c, g, d_seen, CoverCount{d_covered});
        MK_HIP(hipGetLastError());
    }
    if (d_cells) {
        const uint64_t nvec = cover_table_bytes(c) / 16;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(2048, (nvec + 255) / 256);
        hipLaunchKernelGGL(cover_cells_kernel, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(d_seen), nvec, d_cells);
        MK_HIP(hipGetLastError());
    }
    return MK_OK;
}

// Two bytes: slots per LDS range.  16,384 (64 KiB and the list: two workgroups per CU) unless MIEKKI_WIN_VALUES says otherwise: a
// power of two from 256 on, as large as one workgroup's LDS holds beside the list (32,768).
constexpr uint32_t kWinValuesMax = 32768;
static size_t cover_win_lds(uint32_t values) { return ((size_t)values + kWinList + 4) * 4; }

int cover_win_values(const mk_ctx *c, uint32_t *values)
{
    uint32_t v = c->W == 1 ? 256u : 16384u;
    if (c->W == 2)
        if (const char *e = getenv("MIEKKI_WIN_VALUES")) {
            const long x = atol(e);
            if (x < 256 || x > (long)kWinValuesMax || (x & (x - 1))) {
                set_error("MIEKKI_WIN_VALUES takes a power of two from 256 to %u: a larger range does not fit the workgroup's LDS", kWinValuesMax);
                return MK_ERR_ARG;
            }
            v = (uint32_t)x;
        }
    if (values) *values = v;
    return MK_OK;
}

// Rows per workgroup: about 2,048 workgroups, and at least 4 rows (a row per wave at one byte; at two the first clearing of the
// table stands against 4 rows).  MIEKKI_WIN_ROWS: the tests make small indexes take chunks of any size.
static uint32_t cover_win_rows(const mk_ctx *c)
{
    uint64_t rows = std::max<uint64_t>(4, ((uint64_t)c->P + 2047) / 2048);
    if (const char *e = getenv("MIEKKI_WIN_ROWS")) { const long v = atol(e); if (v >= 1) rows = (uint64_t)v; }
    return (uint32_t)std::min<uint64_t>(rows, c->P);
}

// MIEKKI_WIN_TOUCHED=0 / 1: two bytes, the whole range read out and cleared per row / the touched slots only (tools/winners_rate.py
// measures both)
// MIEKKI_WIN_FILTER=0 / 1: the LDS atomic without / with the plain read in front of it (likewise)
static uint32_t cover_win_flags()
{
    uint32_t flags = kWinTouched;
    if (const char *e = getenv("MIEKKI_WIN_TOUCHED")) flags = atol(e) != 0 ? kWinTouched : 0u;
    if (const char *e = getenv("MIEKKI_WIN_FILTER")) if (atol(e) == 0) flags |= kWinNoFilter;
    return flags;
}

// d_won[G] is ADDED to: the caller zeroes it.  d_rank[G]: 0 = best; d_order[G]: its inverse.  Raw cold rows.
int launch_cover_win(mk_ctx *c, const uint32_t *d_seen, const uint32_t *d_rank, const uint32_t *d_order, uint32_t *d_won)
{
    if (!c->G) return MK_OK;
    uint32_t values = 0, ntiles = 0;
    MK_TRY(cover_win_values(c, &values));
    MK_TRY(row_tiles(c, &ntiles));
    const uint32_t rows = cover_win_rows(c), chunks = (c->P + rows - 1) / rows, flags = cover_win_flags();
    const dim3 grid(chunks), block(256);
    if (c->W == 1) {
        hipLaunchKernelGGL(cover_win_kernel<1>, grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, c->G, ntiles, rows, values, flags, d_seen, d_rank, d_order, d_won);
    } else {
        MK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(cover_win_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cover_win_lds(kWinValuesMax)));
        hipLaunchKernelGGL(cover_win_kernel<2>, grid, block, cover_win_lds(values), c->stream, mat_ref(c), c->ld, c->P, c->G, ntiles, rows, values, flags, d_seen, d_rank, d_order, d_won);
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
