// K6i: a panel -- the breadth of coverage (cover.hip) of up to eight samples with ONE pass over the matrix.
//
// With seen_s, covered_s and cells_s the cover's seen, covered and cells for sample Q_s (cover.hip), s < MK_PANEL_SLOTS = 8:
//   table          one byte per (partition, fingerprint value), byte (p << fp_bits) + v, P << fp_bits bytes of caller-owned
//                  device memory (the size of a depth table); bit s of the byte is set iff seen_s(p, v)
//   covered[s][g]  covered_s(g)
//   cells[s]       cells_s
// Integers only, no thresholds; marks accumulate by OR, a pass made twice changes nothing, and nothing depends on chunks, launch
// order or how a sample is cut into sets.  The 8-bit noise floor of the cover holds per slot.
//
//   mark:   table_pass.hpp's walks; the cell operation ORs bit 8 * (cell & 3) + slot into the containing dword: a relaxed
//           agent-scope atomic for the reasons cover.hip's `mark` gives, the slot a template parameter (the walks' cell operation
//           takes the table and the cell, nothing else).  FILTER: a plain load in front, the atomic skipped when the bit already
//           reads 1 -- bits are never cleared inside a pass, so a 1 cannot be stale.
//   count:  the shape of table_pass_kernel -- a wave owns T tiles of 1 KiB of a row, 16 bytes per lane, a workgroup a chunk of
//           rows, the next group's loads in flight, the byte table staged through LDS as depth.hip's is at one-byte fingerprints
//           (the 256-byte slices of 32 rows, double buffered, `empty`'s byte cleared on the way in) and looked up where it lies at
//           two (`empty` skipped by value) -- with another accumulator.  One byte lookup per stored fingerprint is the eight
//           samples' mask; four genomes' bytes make a mask word, bit 8 b + s = sample s against genome byte b, and the mask words
//           of successive rows are COUNTED in bit planes as scan_dense_lut_kernel counts its own: a group of RG rows goes in
//           through carry-save adders (v_bitop3: parity and majority), the carry of weight RG ripples through the planes below
//           256, and what falls out of those waits in a pending word -- a counter passes a multiple of 256 at most once in 256
//           rows -- which goes through the upper planes once per 256 rows.  A lane has four mask words at either width (T = 1
//           at one byte, 2 at two) and groups of RG = 4 rows.  kPanelPlanes = 12: a counter holds 4,095, a chunk has at most
//           that many rows (whole stages where staged: 4,064), which the host enforces through table_pass_grid's rows_cap.
//           Planes cost four registers each: with 12 the kernel takes 106 VGPRs at one byte and 126 at two, four waves per
//           SIMD at both; 13 planes (130 at two bytes) or groups of eight rows at one byte (154) lose a wave, and a chunk of
//           4,095 rows still stands for 4 MiB of a wave's rows against its 16 x 8 adds.  4 x (8 + 4 + 1) = 52 registers
//           of counters.  At the end of the chunk the planes become numbers, slot by slot, and every (slot < n_slots, genome < G)
//           with a count gets one relaxed agent-scope add into covered[slot * G + genome].  Columns [G, pitch) are zero padding:
//           they collect the counts of cell (p, 0) and are never added anywhere.
//   cells:  a reduction over the table, eight popcounts per dword (x & (0x01010101 << s)).
//   slot:   one slot's plane as a cover table: 32 panel bytes become one 32-bit word.
#include <algorithm>
#include <cstdlib>

#include "table_pass.hpp"

namespace mk {

namespace {

template <bool FILTER, uint32_t SLOT>
__device__ __forceinline__ void panel_or(uint8_t *__restrict__ panel, uint64_t cell)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(panel + (cell & ~3ull));
    const uint32_t m = 1u << (((uint32_t)cell & 3u) * 8u + SLOT);
    if (FILTER && (*w & m)) return;
    (void)__hip_atomic_fetch_or(w, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <uint32_t SLOT>
int launch_panel_mark_slot(mk_ctx *c, const mk_qset *qs, bool filter, uint8_t *d_panel)
{
    return launch_table_mark<uint8_t, panel_or<false, SLOT>, panel_or<true, SLOT>>(c, qs, filter, d_panel);
}

// the table of mask bytes as table_pass_grid sees it (depth.hip's ByteTable has the same shape)
struct PanelTable {
    using Cell = uint8_t;
    static constexpr uint32_t kCellBits = 8;
};

// sum and carry of three one-bit inputs per bit position (scan_kernel.hpp's csa: two v_bitop3_b32)
__device__ __forceinline__ void csa(uint32_t &carry, uint32_t &sum, uint32_t a, uint32_t b, uint32_t c)
{
    carry = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
    sum = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

constexpr uint32_t kPanelPlanes = 12, kPanelLow = 8, kPanelUp = kPanelPlanes - kPanelLow;
constexpr uint32_t kPanelMaxRows = (1u << kPanelPlanes) - 1u;             // what a counter holds

template <int W>
struct PanelShape {
    static constexpr uint32_t T = W == 1 ? 1 : 2, RG = 4;                 // tiles per wave, rows per group: T x RG loads in flight
    static constexpr uint32_t kSliceVec = (8u << (8 * W)) / 128u;          // uint4s of one row's slice
    static constexpr bool kStaged = kSliceVec <= kStageVec;
    static constexpr uint32_t kStageRows = kStaged ? kStageVec / kSliceVec : 1u;
    static constexpr uint32_t kTileWords = 4u / W, kWords = T * kTileWords;        // mask words of a lane: per tile, in all
    static constexpr uint32_t kRowsCap = kPanelMaxRows / kStageRows * kStageRows;   // whole stages
    static_assert(!kStaged || kStageRows % RG == 0, "a group of rows lies in one stage");
    static_assert(256u % RG == 0, "the pending carries go up after whole groups");
};

template <int W>
__global__ __launch_bounds__(256) void panel_count_kernel(MatRef M, uint64_t ld, uint32_t P, uint32_t G, uint32_t ntiles, uint32_t rows_per_chunk,
                                                          uint32_t n_slots, const uint8_t *__restrict__ table, uint32_t *__restrict__ covered)
{
    using S = PanelShape<W>;
    constexpr uint32_t T = S::T, RG = S::RG, kSliceVec = S::kSliceVec, kStageRows = S::kStageRows, kTileWords = S::kTileWords, kWords = S::kWords;
    constexpr bool kStaged = S::kStaged;
    constexpr uint32_t kSliceCells = kSliceVec * 16u, kPerLane = 16u / W;
    __shared__ uint4 s_tab[kStaged ? 2 : 1][kStaged ? kStageVec : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tile0 = (blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(tid >> 6)) * T;
    const uint32_t r_lo = blockIdx.y * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);          // (rows_per_chunk <= kRowsCap)
    const uint32_t nrows = r_hi - r_lo, ngroups = (nrows + RG - 1) / RG, nstages = (nrows + kStageRows - 1) / kStageRows;
    const uint64_t tab_vec = (uint64_t)P * kSliceVec;
    const uint4 *__restrict__ table4 = reinterpret_cast<const uint4 *>(table);

    // the table's stages, as table_pass_kernel takes them
    uint4 tv[2];
    auto fetch = [&](uint32_t s) {
        const uint64_t base = ((uint64_t)r_lo + (uint64_t)s * kStageRows) * kSliceVec;
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint64_t idx = base + tid + 256u * u;
            tv[u] = idx < tab_vec ? table4[idx] : make_uint4(0, 0, 0, 0);  // (a stage may reach past the chunk, never past the table)
        }
    };
    auto put = [&](uint32_t b) {
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint32_t j = tid + 256u * u;
            uint4 x = tv[u];
            if ((j & (kSliceVec - 1u)) == kSliceVec - 1u) x.w &= 0x00ffffffu;          // the slice's last byte is `empty`'s
            s_tab[b][j] = x;
        }
    };
    uint4 cur[RG][T], nxt[RG][T];
    auto load = [&](uint32_t g, uint4 (&m)[RG][T]) {
#pragma unroll
        for (uint32_t u = 0; u < RG; ++u) {
            const uint32_t r = min(r_lo + g * RG + u, r_hi - 1u);            // (every load goes out; rows past the chunk are not counted)
#pragma unroll
            for (uint32_t t = 0; t < T; ++t)
                if (tile0 + t < ntiles)                                    // (wave-uniform; ld covers whole tiles)
                    m[u][t] = *reinterpret_cast<const uint4 *>(mat_row(M, r, ld) + (uint64_t)(tile0 + t) * kTileBytes + lane * 16u);
                else
                    m[u][t] = make_uint4(0, 0, 0, 0);
        }
    };
    // low[w][k]: bit k of the counters of mask word w, k < 8; up[w][k]: bit 8 + k; pend[w]: carries of weight 256 on their way up
    uint32_t low[kWords][kPanelLow], up[kWords][kPanelUp], pend[kWords];
#pragma unroll
    for (uint32_t w = 0; w < kWords; ++w) {
        pend[w] = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPanelLow; ++k) low[w][k] = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPanelUp; ++k) up[w][k] = 0;
    }
    auto flush_pending = [&]() {
#pragma unroll
        for (uint32_t w = 0; w < kWords; ++w) {
            uint32_t c = pend[w];
            pend[w] = 0;
#pragma unroll
            for (uint32_t k = 0; k < kPanelUp; ++k) {
                const uint32_t t = up[w][k];
                up[w][k] = t ^ c;
                c &= t;
            }
        }
    };

    if constexpr (kStaged) {
        fetch(0);
        put(0);
    }
    load(0, cur);
    if constexpr (kStaged) __syncthreads();
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t row = g * RG, s = row / kStageRows;                 // the group's first row in the chunk, its stage
        const bool first = row % kStageRows == 0, last = (row + RG) % kStageRows == 0 || g + 1 == ngroups;
        if constexpr (kStaged)
            if (first && s + 1 < nstages) fetch(s + 1);
        if (g + 1 < ngroups) load(g + 1, nxt);
        const uint8_t *tab;
        if constexpr (kStaged) tab = reinterpret_cast<const uint8_t *>(s_tab[s & 1u]) + (row - s * kStageRows) * kSliceCells;
        else tab = table + (uint64_t)(r_lo + row) * kSliceCells;
#pragma unroll
        for (uint32_t t = 0; t < T; ++t) {
            if (tile0 + t >= ntiles) continue;                             // (wave-uniform: its counters stay zero)
#pragma unroll
            for (uint32_t x = 0; x < kTileWords; ++x) {
                // the group's mask words of this lane's genomes 4 x .. 4 x + 3 of tile t; a row past the chunk gives none
                uint32_t m[RG];
#pragma unroll
                for (uint32_t u = 0; u < RG; ++u) {
                    m[u] = 0;
                    if (row + u >= nrows) continue;                        // (uniform)
                    const uint8_t *sl = tab + (size_t)u * kSliceCells;
                    const uint32_t d[4] = {cur[u][t].x, cur[u][t].y, cur[u][t].z, cur[u][t].w};
                    if constexpr (W == 1) {
                        const uint32_t v = d[x];                           // (a staged slice holds 0 at `empty`)
                        m[u] = (uint32_t)sl[v & 255u] | (uint32_t)sl[(v >> 8) & 255u] << 8 | (uint32_t)sl[(v >> 16) & 255u] << 16 | (uint32_t)sl[v >> 24] << 24;
                    } else {
#pragma unroll
                        for (uint32_t b = 0; b < 4; ++b) {
                            const uint32_t v = (d[x * 2 + b / 2] >> (16u * (b & 1u))) & 65535u;
                            const uint32_t cell = sl[v];                   // (every lane loads: `empty`'s byte lies in the table too)
                            m[u] |= (v == 65535u ? 0u : cell) << (8u * b);
                        }
                    }
                }
                uint32_t (&p)[kPanelLow] = low[t * kTileWords + x];
                // four rows in: three adders of two instructions each
                static_assert(RG == 4, "the adder tree that is written out");
                uint32_t t0, t1, carry;
                csa(t0, p[0], p[0], m[0], m[1]);
                csa(t1, p[0], p[0], m[2], m[3]);
                csa(carry, p[1], p[1], t0, t1);
                // one bit of weight four per position: through the planes up to 128, what falls out of them waits in `pend`
#pragma unroll
                for (uint32_t k = 2; k < kPanelLow; ++k) {
                    const uint32_t q = p[k];
                    p[k] = q ^ carry;
                    carry &= q;
                }
                pend[t * kTileWords + x] |= carry;
            }
        }
        if ((row + RG) % 256u == 0) flush_pending();                       // (256 rows since the last time: uniform)
        if constexpr (kStaged) {
            // the next stage's slices go into the other buffer: everybody left it at the barrier that ended the stage before
            if (last && s + 1 < nstages) put((s + 1) & 1u);
            if (last) __syncthreads();
        }
#pragma unroll
        for (uint32_t u = 0; u < RG; ++u)
#pragma unroll
            for (uint32_t t = 0; t < T; ++t) cur[u][t] = nxt[u][t];
    }
    flush_pending();
    // the planes -> numbers, slot by slot, four genomes of a word at a time: the low eight planes into byte counters, the upper
    // planes into a second set (four planes: the upper count stays below 16)
#pragma unroll
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t g0 = (tile0 + t) * (kTileBytes / W) + lane * kPerLane;      // (tile0 + t >= ntiles: g0 >= G)
        if (g0 >= G) continue;
#pragma unroll
        for (uint32_t j = 0; j < MK_PANEL_SLOTS; ++j) {
            if (j >= n_slots) break;                                       // (uniform)
            uint32_t *__restrict__ out = covered + (size_t)j * G + g0;
#pragma unroll
            for (uint32_t x = 0; x < kTileWords; ++x) {
                const uint32_t w = t * kTileWords + x;
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (uint32_t k = 0; k < kPanelLow; ++k) lo += ((low[w][k] >> j) & 0x01010101u) << k;
#pragma unroll
                for (uint32_t k = 0; k < kPanelUp; ++k) hi += ((up[w][k] >> j) & 0x01010101u) << k;
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint32_t n = ((lo >> (8u * b)) & 255u) | (((hi >> (8u * b)) & 255u) << 8);
                    const uint32_t gi = x * 4u + b;
                    if (n && g0 + gi < G) (void)__hip_atomic_fetch_add(out + gi, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (columns [G, pitch) are padding)
                }
            }
        }
    }
}

// cells[s] += the table's bytes with bit s set
__global__ __launch_bounds__(256) void panel_cells_kernel(const uint4 *__restrict__ panel4, uint64_t nvec, unsigned long long *__restrict__ cells)
{
    uint32_t n[MK_PANEL_SLOTS];
#pragma unroll
    for (uint32_t s = 0; s < MK_PANEL_SLOTS; ++s) n[s] = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nvec; i += (uint64_t)gridDim.x * 256u) {
        const uint4 x = panel4[i];
        // (a lane's share stays far below 2^32: at most 2^44 bytes over 2^19 lanes)
#pragma unroll
        for (uint32_t s = 0; s < MK_PANEL_SLOTS; ++s) {
            const uint32_t m = 0x01010101u << s;
            n[s] += __popc(x.x & m) + __popc(x.y & m) + __popc(x.z & m) + __popc(x.w & m);
        }
    }
#pragma unroll
    for (uint32_t s = 0; s < MK_PANEL_SLOTS; ++s) {
        uint64_t total = n[s];
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
        if ((threadIdx.x & 63u) == 0 && total) (void)__hip_atomic_fetch_add(cells + s, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// bit `slot` of four bytes as a nibble, byte b's at bit b (the products' bits do not meet: no carries)
__device__ __forceinline__ uint32_t slot_nibble(uint32_t x, uint32_t slot) { return (((x >> slot) & 0x01010101u) * 0x01020408u) >> 24; }

// seen[i] = bit `slot` of panel bytes 32 i .. 32 i + 31
__global__ __launch_bounds__(256) void panel_slot_kernel(const uint4 *__restrict__ panel4, uint64_t nwords, uint32_t slot, uint32_t *__restrict__ seen)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * 256u) {
        const uint4 a = panel4[i * 2], b = panel4[i * 2 + 1];
        seen[i] = slot_nibble(a.x, slot) | slot_nibble(a.y, slot) << 4 | slot_nibble(a.z, slot) << 8 | slot_nibble(a.w, slot) << 12 |
                  slot_nibble(b.x, slot) << 16 | slot_nibble(b.y, slot) << 20 | slot_nibble(b.z, slot) << 24 | slot_nibble(b.w, slot) << 28;
    }
}

}  // namespace

uint64_t panel_table_bytes(const mk_ctx *c) { return (uint64_t)c->P << c->p.fp_bits; }

int launch_panel_reset(mk_ctx *c, uint8_t *d_panel)
{
    MK_HIP(hipMemsetAsync(d_panel, 0, panel_table_bytes(c), c->stream));
    return MK_OK;
}

// MIEKKI_PANEL_FILTER=0 / 1: the marks without / with the plain load in front of the atomic (tools/panel_rate.py measures both)
static bool panel_filter()
{
    if (const char *e = getenv("MIEKKI_PANEL_FILTER")) return atol(e) != 0;
    return true;
}

int launch_panel_mark(mk_ctx *c, const mk_qset *qs, uint32_t slot, uint8_t *d_panel)
{
    const bool filter = panel_filter();
    switch (slot) {
    case 0: return launch_panel_mark_slot<0>(c, qs, filter, d_panel);
    case 1: return launch_panel_mark_slot<1>(c, qs, filter, d_panel);
    case 2: return launch_panel_mark_slot<2>(c, qs, filter, d_panel);
    case 3: return launch_panel_mark_slot<3>(c, qs, filter, d_panel);
    case 4: return launch_panel_mark_slot<4>(c, qs, filter, d_panel);
    case 5: return launch_panel_mark_slot<5>(c, qs, filter, d_panel);
    case 6: return launch_panel_mark_slot<6>(c, qs, filter, d_panel);
    case 7: return launch_panel_mark_slot<7>(c, qs, filter, d_panel);
    }
    set_error("panel slot %u: a panel has %u slots", slot, MK_PANEL_SLOTS);
    return MK_ERR_ARG;
}

// d_covered[n_slots][G] and d_cells[8] are ADDED to (either may be null): the caller zeroes them; raw cold rows.  A chunk has
// at most as many rows as a counter of kPanelPlanes planes holds: MIEKKI_PANEL_ROWS above that is clamped.
int launch_panel_count(mk_ctx *c, const uint8_t *d_panel, uint32_t n_slots, uint32_t *d_covered, unsigned long long *d_cells)
{
    if (d_covered && c->G) {
        PassGrid g;
        // about 1,024 workgroups, one round of the device at four waves per SIMD, where the cover's pass takes 2,048: a chunk's
        // read-out is up to eight adds per genome (20,000 genomes at -h 17, tools/panel_rate.py: chunks of 352 rows 3.4 ms at one
        // byte, of 704 rows 2.4, of 1,408 rows 2.1, of 2,816 rows 2.5; at two bytes 192 rows 6.4 ms, 704 rows 5.0, 1,408 rows 5.3)
        MK_TRY(table_pass_grid<PanelTable>(c, "MIEKKI_PANEL_ROWS", &g, c->W == 1 ? PanelShape<1>::kRowsCap : PanelShape<2>::kRowsCap, 1024,
                                           c->W == 1 ? PanelShape<1>::T : PanelShape<2>::T));
        const dim3 grid(g.columns, g.chunks), block(256);
        if (c->W == 1) hipLaunchKernelGGL(panel_count_kernel<1>, grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, c->G, g.ntiles, g.rows, n_slots, d_panel, d_covered);
        else hipLaunchKernelGGL(panel_count_kernel<2>, grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, c->G, g.ntiles, g.rows, n_slots, d_panel, d_covered);
        MK_HIP(hipGetLastError());
    }
    if (d_cells) {
        const uint64_t nvec = panel_table_bytes(c) / 16;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>(2048, (nvec + 255) / 256);
        hipLaunchKernelGGL(panel_cells_kernel, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(d_panel), nvec, d_cells);
        MK_HIP(hipGetLastError());
    }
    return MK_OK;
}

// d_seen (cover_table_bytes) is WRITTEN
int launch_panel_slot(mk_ctx *c, const uint8_t *d_panel, uint32_t slot, uint32_t *d_seen)
{
    const uint64_t nwords = panel_table_bytes(c) / 32;
    if (!nwords) return MK_OK;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1u << 20, (nwords + 255) / 256);
    hipLaunchKernelGGL(panel_slot_kernel, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(d_panel), nwords, slot, d_seen);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
