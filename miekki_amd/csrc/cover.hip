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
//   mark:   the set's gated sketch OR-ed into the table.  One wave per sparse query walks its entry list (partition in the low
//           word, fingerprint in the high word); dense queries and column sets: one lane per (group, partition) of
//           dense[group][p][4], empty slots skipped.  Waves on every XCD OR into the same words and the per-XCD L2s are not
//           coherent, so -- as for tally.hip's counters -- every mark is an agent-scope atomic; relaxed, because nothing reads
//           the table inside the pass and the result of the OR is not used; later launches and copies on the stream see it.
//           FILTER: a plain load in front of the atomic, which is skipped when the bit already reads 1.  A stale 0 costs an
//           atomic; a 1 cannot be stale, bits are never cleared inside a pass.
//   count:  one streaming pass over the matrix, every row read once (hot and cold rows alike, mat_row).  A workgroup owns
//           4 x T tiles (a wave: T tiles of 1 KiB of a row, 16 bytes per lane) and a chunk of rows.  The table goes through
//           LDS 8 KiB at a time, double buffered: the slices of 256 rows at one byte per fingerprint (32 B each), the slice of
//           one row at two (8 KiB) -- with the bit of `empty` cleared on the way in, so that a genome without a fingerprint
//           never counts whatever the table says.  A lane looks each of its fingerprints up with one LDS dword read (one byte:
//           a wave's reads fall on the 8 dwords of one slice, which broadcast; two bytes: random dwords of 2,048) and keeps its
//           genomes' counts in 32-bit registers -- a count reaches P.  The next rows' loads are in flight while a group of rows
//           is looked up.  At the end of the chunk: one relaxed agent-scope add per genome with a count, genomes below G only
//           (columns [G, pitch) of a row are zero padding and would read seen(p, 0)).
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

#include "mk_internal.hpp"

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

template <bool FILTER>
__global__ __launch_bounds__(256) void cover_mark_sparse_kernel(const uint64_t *__restrict__ entries, const uint64_t *__restrict__ ent_off,
                                                                const uint32_t *__restrict__ scan_n, uint32_t nq, uint32_t P, uint32_t fp_bits,
                                                                uint32_t empty, uint32_t *__restrict__ seen)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= nq) return;
    const uint32_t n = scan_n[q];                                          // (0 for the dense queries: their slots are walked below)
    const uint64_t *__restrict__ e = entries + ent_off[q];
    for (uint32_t i = lane; i < n; i += 64u) {
        const uint64_t ent = e[i];
        const uint32_t p = (uint32_t)ent, v = (uint32_t)(ent >> 32);
        if (p < P && v < empty) mark<FILTER>(seen, ((uint64_t)p << fp_bits) + v);
    }
}

template <int W, bool FILTER>
__global__ __launch_bounds__(256) void cover_mark_dense_kernel(const uint8_t *__restrict__ dense, uint64_t n, uint32_t P, uint32_t *__restrict__ seen)
{
    constexpr uint32_t kBits = 8 * W, kEmpty = (1u << kBits) - 1u;
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;          // (group, partition): four slots of W bytes
    if (i >= n) return;
    const uint32_t p = (uint32_t)(i & (P - 1u));
    uint32_t w[W];
#pragma unroll
    for (int k = 0; k < W; ++k) w[k] = reinterpret_cast<const uint32_t *>(dense)[i * W + k];
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t v = (w[s * W / 4] >> ((s * kBits) & 31u)) & kEmpty;
        if (v != kEmpty) mark<FILTER>(seen, ((uint64_t)p << kBits) + v);
    }
}

constexpr uint32_t kStageDwords = 2048;   // the table goes through LDS 8 KiB at a time

template <int W> struct CoverShape;
template <> struct CoverShape<1> { static constexpr uint32_t T = 1, RU = 8; };   // tiles per wave, rows in flight per wave
template <> struct CoverShape<2> { static constexpr uint32_t T = 4, RU = 1; };

template <int W>
__global__ __launch_bounds__(256) void cover_count_kernel(MatRef M, uint64_t ld, uint32_t P, uint32_t G, uint32_t ntiles, uint32_t rows_per_chunk,
                                                          const uint32_t *__restrict__ seen, uint32_t *__restrict__ covered)
{
    constexpr uint32_t T = CoverShape<W>::T, RU = CoverShape<W>::RU;
    constexpr uint32_t kBits = 8 * W, kMask = (1u << kBits) - 1u, kSliceVec = (1u << kBits) / 128u;    // uint4s of one row's slice
    constexpr uint32_t kStageRows = kStageDwords / 4u / kSliceVec, kPerLane = 16u / W;
    static_assert(kStageRows % RU == 0, "a group of rows lies in one stage");
    __shared__ uint4 s_tab[2][kStageDwords / 4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tile0 = (blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(tid >> 6)) * T;
    const uint32_t r_lo = blockIdx.y * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);          // (rows_per_chunk <= P <= 2^28)
    const uint32_t nrows = r_hi - r_lo, ngroups = (nrows + RU - 1) / RU, nstages = (nrows + kStageRows - 1) / kStageRows;
    const uint64_t tab_vec = (uint64_t)P * kSliceVec;
    const uint4 *__restrict__ seen4 = reinterpret_cast<const uint4 *>(seen);

    uint4 tv[2];
    auto fetch = [&](uint32_t s) {
        const uint64_t base = ((uint64_t)r_lo + (uint64_t)s * kStageRows) * kSliceVec;
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint64_t idx = base + tid + 256u * u;
            tv[u] = idx < tab_vec ? seen4[idx] : make_uint4(0, 0, 0, 0);   // (a stage may reach past the chunk, never past the table)
        }
    };
    auto put = [&](uint32_t b) {
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint32_t j = tid + 256u * u;
            uint4 x = tv[u];
            if ((j & (kSliceVec - 1u)) == kSliceVec - 1u) x.w &= 0x7fffffffu;   // the slice's last bit is `empty`'s
            s_tab[b][j] = x;
        }
    };
    uint4 cur[RU][T], nxt[RU][T];
    auto load = [&](uint32_t g, uint4 (&m)[RU][T]) {
#pragma unroll
        for (uint32_t u = 0; u < RU; ++u) {
            const uint32_t r = min(r_lo + g * RU + u, r_hi - 1u);            // (every load goes out; rows past the chunk are not counted)
#pragma unroll
            for (uint32_t t = 0; t < T; ++t)
                if (tile0 + t < ntiles)                                    // (wave-uniform; ld covers whole tiles)
                    m[u][t] = *reinterpret_cast<const uint4 *>(mat_row(M, r, ld) + (uint64_t)(tile0 + t) * kTileBytes + lane * 16u);
        }
    };
    uint32_t cnt[T][kPerLane];
#pragma unroll
    for (uint32_t t = 0; t < T; ++t)
#pragma unroll
        for (uint32_t j = 0; j < kPerLane; ++j) cnt[t][j] = 0;

    fetch(0);
    put(0);
    load(0, cur);
    __syncthreads();
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t row = g * RU, s = row / kStageRows;                 // the group's first row in the chunk, its stage
        const bool first = row % kStageRows == 0, last = (row + RU) % kStageRows == 0 || g + 1 == ngroups;
        if (first && s + 1 < nstages) fetch(s + 1);
        if (g + 1 < ngroups) load(g + 1, nxt);
        const uint32_t *tab = reinterpret_cast<const uint32_t *>(s_tab[s & 1u]) + (row - s * kStageRows) * (kSliceVec * 4u);
#pragma unroll
        for (uint32_t u = 0; u < RU; ++u) {
            if (row + u >= nrows) break;                                   // (uniform)
            const uint32_t *sl = tab + u * (kSliceVec * 4u);
#pragma unroll
            for (uint32_t t = 0; t < T; ++t) {
                if (tile0 + t >= ntiles) continue;
                const uint32_t w[4] = {cur[u][t].x, cur[u][t].y, cur[u][t].z, cur[u][t].w};
#pragma unroll
                for (uint32_t j = 0; j < kPerLane; ++j) {
                    const uint32_t v = (w[j * W / 4] >> ((j * kBits) & 31u)) & kMask;
                    cnt[t][j] += (sl[v >> 5] >> (v & 31u)) & 1u;
                }
            }
        }
        // the next stage's slices go into the other buffer: everybody left it at the barrier that ended the stage before
        if (last && s + 1 < nstages) put((s + 1) & 1u);
        if (last) __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < RU; ++u)
#pragma unroll
            for (uint32_t t = 0; t < T; ++t) cur[u][t] = nxt[u][t];
    }
#pragma unroll
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t g0 = (tile0 + t) * (kTileBytes / W) + lane * kPerLane;      // (tile0 + t >= ntiles: g0 >= G)
#pragma unroll
        for (uint32_t j = 0; j < kPerLane; ++j)
            if (g0 + j < G && cnt[t][j]) (void)__hip_atomic_fetch_add(covered + g0 + j, cnt[t][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

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

// lanes of one wave exchange LDS values: what was written before is visible after (LDS serves a wave's accesses in order)
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
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
    if (!qs->nq) return MK_OK;
    const bool filter = cover_filter();
    if (!qs->columns) {
        const dim3 grid((qs->nq + 3) / 4), block(256);
        if (filter) hipLaunchKernelGGL(cover_mark_sparse_kernel<true>, grid, block, 0, c->stream, qs->d_entries, qs->d_ent_off, qs->d_scan_n, qs->nq, c->P, c->p.fp_bits, c->empty, d_seen);
        else hipLaunchKernelGGL(cover_mark_sparse_kernel<false>, grid, block, 0, c->stream, qs->d_entries, qs->d_ent_off, qs->d_scan_n, qs->nq, c->P, c->p.fp_bits, c->empty, d_seen);
    }
    if (!qs->dense_q.empty()) {
        const uint64_t n = (uint64_t)(qs->dense_q.size() / 4) * c->P, blocks = (n + 255) / 256;
        if (blocks > 0x7fffffffull) { set_error("too many dense queries for one mark pass"); return MK_ERR_ARG; }
        const dim3 grid((uint32_t)blocks), block(256);
        if (c->W == 1) {
            if (filter) hipLaunchKernelGGL((cover_mark_dense_kernel<1, true>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_seen);
            else hipLaunchKernelGGL((cover_mark_dense_kernel<1, false>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_seen);
        } else {
            if (filter) hipLaunchKernelGGL((cover_mark_dense_kernel<2, true>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_seen);
            else hipLaunchKernelGGL((cover_mark_dense_kernel<2, false>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_seen);
        }
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// Rows per chunk: enough workgroups to fill the device several times over (2,048), whole stages of the table, and at least 256
// (64) rows, so that a genome's add at the end of a chunk stands against 256 (128) bytes read.  MIEKKI_COVER_ROWS: the tests
// make small indexes take several chunks, whole stages or not.
static uint32_t cover_rows_per_chunk(const mk_ctx *c, uint32_t columns)
{
    const uint32_t stage_rows = c->W == 1 ? kStageDwords / 8u : 1u, least = c->W == 1 ? 256u : 64u;
    const uint64_t chunks = std::max<uint64_t>(1, 2048 / columns);
    uint64_t rows = std::max<uint64_t>(least, (c->P + chunks - 1) / chunks);
    rows = (rows + stage_rows - 1) / stage_rows * stage_rows;
    if (const char *e = getenv("MIEKKI_COVER_ROWS")) { const long v = atol(e); if (v >= 1) rows = (uint64_t)v; }
    return (uint32_t)std::min<uint64_t>(rows, c->P);
}

// d_covered[G] and *d_cells are ADDED to: the caller zeroes them
int launch_cover_count(mk_ctx *c, const uint32_t *d_seen, uint32_t *d_covered, unsigned long long *d_cells)
{
    if (d_covered && c->G) {
        const uint32_t ntiles = (uint32_t)(((uint64_t)c->G * c->W + kTileBytes - 1) / kTileBytes);
        if ((uint64_t)ntiles * kTileBytes > c->ld) { set_error("the matrix rows do not cover whole tiles"); return MK_ERR_STATE; }
        const uint32_t per_wg = 4u * (c->W == 1 ? CoverShape<1>::T : CoverShape<2>::T), columns = (ntiles + per_wg - 1) / per_wg;
        const uint32_t rows = cover_rows_per_chunk(c, columns), chunks = (c->P + rows - 1) / rows;
        if (chunks > 65535u) { set_error("MIEKKI_COVER_ROWS cuts the rows into more than 65,535 chunks"); return MK_ERR_ARG; }
        const dim3 grid(columns, chunks), block(256);
        if (c->W == 1) hipLaunchKernelGGL(cover_count_kernel<1>, grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, c->G, ntiles, rows, d_seen, d_covered);
        else hipLaunchKernelGGL(cover_count_kernel<2>, grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, c->G, ntiles, rows, d_seen, d_covered);
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
    uint32_t values = 0;
    MK_TRY(cover_win_values(c, &values));
    const uint32_t ntiles = (uint32_t)(((uint64_t)c->G * c->W + kTileBytes - 1) / kTileBytes);
    if ((uint64_t)ntiles * kTileBytes > c->ld) { set_error("the matrix rows do not cover whole tiles"); return MK_ERR_STATE; }
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
