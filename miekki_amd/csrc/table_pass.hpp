// What cover.hip and depth.hip share: a table of one cell per (partition, fingerprint value) in caller-owned device memory -- a
// bit (`seen`) or a byte (`mult`), cell (p << fp_bits) + v -- the walks that mark a set's gated sketch in it, and the streaming
// pass over the matrix that looks every stored fingerprint up in it.  A table says what a cell is (Table, below); a pass says
// what it keeps per genome (Acc).
//
//   mark:  one wave per sparse query walks its entry list (partition in the low word, fingerprint in the high word); dense
//          queries and column sets: one lane per (group, partition) of dense[group][p][4], empty slots skipped.  What a mark
//          does to its cell, and why that is safe from every XCD at once, stands with the cell operations: cover.hip's `mark`,
//          depth.hip's `bump`, panel.hip's `panel_or` (whose count pass is a kernel of its own on table_pass_grid's chunks).
//   pass:  every row read once (hot and cold rows alike, mat_row).  A workgroup owns 4 x T tiles (a wave: T tiles of 1 KiB of
//          a row, 16 bytes per lane) and a chunk of rows, and a lane keeps its genomes' counts in 32-bit registers -- a count
//          reaches P.  The next rows' loads are in flight while a group of RU rows is looked up.  A STAGED table goes through
//          LDS 8 KiB at a time, double buffered: the slices of as many rows as that holds, `empty`'s cell cleared on the way
//          in, so that a genome without a fingerprint never counts whatever the table says.  A table whose row slice is larger
//          than a stage (bytes at two-byte fingerprints: 64 KiB) is looked up where it lies, through L1 / L2, `empty` skipped by
//          value: no LDS, no barrier.  At the end of the chunk the accumulator adds what it kept, genomes below G only (columns
//          [G, pitch) of a row are zero padding and would read cell (p, 0)).
//
//   Table: Cell (what the table pointer points to), kCellBits, clear_empty(uint4 &last) -- the last uint4 of a staged slice,
//          which ends in `empty`'s cell -- and lookup(slice, v).
//   Acc:   the kernel argument that holds the outputs.  A lane keeps two words per genome, a count and a word of the
//          accumulator's own (a sum, a threshold, nothing): start(g, G) gives the second word's first value, add(cnt, aux, m)
//          takes a cell's value m, flush(cnt, aux, g0, j) adds to the outputs of a genome g0 + j < G with a count.  It
//          addresses them as out + g0 + j: a lane's adds then share one base address.  With an address made per genome the
//          two-byte bisection pass came out at 122 VGPRs for 136, a wave more per SIMD, and 6 % slower.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "mk_internal.hpp"

namespace mk {

namespace {

// ---- mark: OP is the cell operation, with or without its filter
template <class Cell, void (*OP)(Cell *, uint64_t)>
__global__ __launch_bounds__(256) void table_mark_sparse_kernel(const uint64_t *__restrict__ entries, const uint64_t *__restrict__ ent_off,
                                                                const uint32_t *__restrict__ scan_n, uint32_t nq, uint32_t P, uint32_t fp_bits,
                                                                uint32_t empty, Cell *__restrict__ table)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= nq) return;
    const uint32_t n = scan_n[q];                                          // (0 for the dense queries: their slots are walked below)
    const uint64_t *__restrict__ e = entries + ent_off[q];
    for (uint32_t i = lane; i < n; i += 64u) {
        const uint64_t ent = e[i];
        const uint32_t p = (uint32_t)ent, v = (uint32_t)(ent >> 32);
        if (p < P && v < empty) OP(table, ((uint64_t)p << fp_bits) + v);
    }
}

template <int W, class Cell, void (*OP)(Cell *, uint64_t)>
__global__ __launch_bounds__(256) void table_mark_dense_kernel(const uint8_t *__restrict__ dense, uint64_t n, uint32_t P, Cell *__restrict__ table)
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
        if (v != kEmpty) OP(table, ((uint64_t)p << kBits) + v);
    }
}

// the marks of a sketched set that is not a shell over parts; PLAIN / FILTERED: the cell operation without / with its filter
template <class Cell, void (*PLAIN)(Cell *, uint64_t), void (*FILTERED)(Cell *, uint64_t)>
int launch_table_mark(mk_ctx *c, const mk_qset *qs, bool filter, Cell *d_table)
{
    if (!qs->nq) return MK_OK;
    if (!qs->columns) {
        const dim3 grid((qs->nq + 3) / 4), block(256);
        if (filter) hipLaunchKernelGGL((table_mark_sparse_kernel<Cell, FILTERED>), grid, block, 0, c->stream, qs->d_entries, qs->d_ent_off, qs->d_scan_n, qs->nq, c->P, c->p.fp_bits, c->empty, d_table);
        else hipLaunchKernelGGL((table_mark_sparse_kernel<Cell, PLAIN>), grid, block, 0, c->stream, qs->d_entries, qs->d_ent_off, qs->d_scan_n, qs->nq, c->P, c->p.fp_bits, c->empty, d_table);
    }
    if (!qs->dense_q.empty()) {
        const uint64_t n = (uint64_t)(qs->dense_q.size() / 4) * c->P, blocks = (n + 255) / 256;
        if (blocks > 0x7fffffffull) { set_error("too many dense queries for one mark pass"); return MK_ERR_ARG; }
        const dim3 grid((uint32_t)blocks), block(256);
        if (c->W == 1) {
            if (filter) hipLaunchKernelGGL((table_mark_dense_kernel<1, Cell, FILTERED>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_table);
            else hipLaunchKernelGGL((table_mark_dense_kernel<1, Cell, PLAIN>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_table);
        } else {
            if (filter) hipLaunchKernelGGL((table_mark_dense_kernel<2, Cell, FILTERED>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_table);
            else hipLaunchKernelGGL((table_mark_dense_kernel<2, Cell, PLAIN>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_table);
        }
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// ---- pass
constexpr uint32_t kStageVec = 512;       // uint4s of a stage: the table goes through LDS 8 KiB at a time

template <int W, class Table>
struct PassShape {
    static constexpr uint32_t T = W == 1 ? 1 : 4, RU = W == 1 ? 8 : 1;     // tiles per wave, rows in flight per wave
    static constexpr uint32_t kSliceVec = (Table::kCellBits << (8 * W)) / 128u;        // uint4s of one row's slice
    static constexpr bool kStaged = kSliceVec <= kStageVec;
    static constexpr uint32_t kStageRows = kStaged ? kStageVec / kSliceVec : 1u;
    static_assert(!kStaged || kStageRows % RU == 0, "a group of rows lies in one stage");
};

template <int W, class Table, class Acc>
__global__ __launch_bounds__(256) void table_pass_kernel(MatRef M, uint64_t ld, uint32_t P, uint32_t G, uint32_t ntiles, uint32_t rows_per_chunk,
                                                         const typename Table::Cell *__restrict__ table, Acc acc)
{
    using Cell = typename Table::Cell;
    using S = PassShape<W, Table>;
    constexpr uint32_t T = S::T, RU = S::RU, kSliceVec = S::kSliceVec, kStageRows = S::kStageRows;
    constexpr bool kStaged = S::kStaged;
    constexpr uint32_t kBits = 8 * W, kMask = (1u << kBits) - 1u, kPerLane = 16u / W;
    constexpr uint32_t kSliceCells = kSliceVec * (16u / sizeof(Cell));     // Cells of one row's slice
    __shared__ uint4 s_tab[kStaged ? 2 : 1][kStaged ? kStageVec : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tile0 = (blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(tid >> 6)) * T;
    const uint32_t r_lo = blockIdx.y * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);          // (rows_per_chunk <= P <= 2^28)
    const uint32_t nrows = r_hi - r_lo, ngroups = (nrows + RU - 1) / RU, nstages = (nrows + kStageRows - 1) / kStageRows;
    const uint64_t tab_vec = (uint64_t)P * kSliceVec;
    const uint4 *__restrict__ table4 = reinterpret_cast<const uint4 *>(table);

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
            if ((j & (kSliceVec - 1u)) == kSliceVec - 1u) Table::clear_empty(x);
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
    // per genome the count and the accumulator's own word (two plain arrays: kept in one struct per genome, the byte pass at
    // one-byte fingerprints took 132 VGPRs instead of 119, a wave less per SIMD)
    uint32_t cnt[T][kPerLane], aux[T][kPerLane];
#pragma unroll
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t g0 = (tile0 + t) * (kTileBytes / W) + lane * kPerLane;
#pragma unroll
        for (uint32_t j = 0; j < kPerLane; ++j) {
            cnt[t][j] = 0;
            aux[t][j] = acc.start(g0 + j, G);
        }
    }

    if constexpr (kStaged) {
        fetch(0);
        put(0);
    }
    load(0, cur);
    if constexpr (kStaged) __syncthreads();
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t row = g * RU, s = row / kStageRows;                 // the group's first row in the chunk, its stage
        const bool first = row % kStageRows == 0, last = (row + RU) % kStageRows == 0 || g + 1 == ngroups;
        if constexpr (kStaged)
            if (first && s + 1 < nstages) fetch(s + 1);
        if (g + 1 < ngroups) load(g + 1, nxt);
        const Cell *tab;
        if constexpr (kStaged) tab = reinterpret_cast<const Cell *>(s_tab[s & 1u]) + (row - s * kStageRows) * kSliceCells;
        else tab = table + (uint64_t)(r_lo + row) * kSliceCells;
#pragma unroll
        for (uint32_t u = 0; u < RU; ++u) {
            if (row + u >= nrows) break;                                   // (uniform)
            const Cell *sl = tab + u * kSliceCells;
#pragma unroll
            for (uint32_t t = 0; t < T; ++t) {
                if (tile0 + t >= ntiles) continue;
                const uint32_t w[4] = {cur[u][t].x, cur[u][t].y, cur[u][t].z, cur[u][t].w};
#pragma unroll
                for (uint32_t j = 0; j < kPerLane; ++j) {
                    const uint32_t v = (w[j * W / 4] >> ((j * kBits) & 31u)) & kMask;
                    // (a staged slice holds 0 at `empty`)
                    Acc::add(cnt[t][j], aux[t][j], !kStaged && v == kMask ? 0u : Table::lookup(sl, v));
                }
            }
        }
        if constexpr (kStaged) {
            // the next stage's slices go into the other buffer: everybody left it at the barrier that ended the stage before
            if (last && s + 1 < nstages) put((s + 1) & 1u);
            if (last) __syncthreads();
        }
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
            if (g0 + j < G && cnt[t][j]) acc.flush(cnt[t][j], aux[t][j], g0, j);               // (columns [G, pitch) are zero padding)
    }
}

// The grid of a pass: a column of workgroups per 4 x T tiles, a chunk of rows each.  Rows per chunk: enough workgroups to fill
// the device several times over (2,048), whole stages of the table, and at least 256 (64) rows, so that a genome's adds at the
// end of a chunk stand against 256 (128) bytes read; `rows_cap` at the most, where the accumulator has a limit.  `rows_switch`
// names the environment variable with which the tests make small indexes take several chunks, whole stages or not.  A pass
// with a kernel of its own (panel.hip) says how many workgroups it aims at and how many tiles its waves take.
struct PassGrid { uint32_t ntiles, columns, rows, chunks; };

template <class Table>
int table_pass_grid(const mk_ctx *c, const char *rows_switch, PassGrid *g, uint64_t rows_cap = ~0ull, uint32_t workgroups = 2048, uint32_t tiles_per_wave = 0)
{
    MK_TRY(row_tiles(c, &g->ntiles));
    const uint32_t per_wg = 4u * (tiles_per_wave ? tiles_per_wave : c->W == 1 ? PassShape<1, Table>::T : PassShape<2, Table>::T);
    const uint32_t stage_rows = c->W == 1 ? PassShape<1, Table>::kStageRows : PassShape<2, Table>::kStageRows, least = c->W == 1 ? 256u : 64u;
    g->columns = (g->ntiles + per_wg - 1) / per_wg;
    const uint64_t chunks = std::max<uint64_t>(1, workgroups / g->columns);
    uint64_t rows = std::max<uint64_t>(least, (c->P + chunks - 1) / chunks);
    rows = (rows + stage_rows - 1) / stage_rows * stage_rows;
    if (const char *e = getenv(rows_switch)) { const long v = atol(e); if (v >= 1) rows = (uint64_t)v; }
    g->rows = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(rows, rows_cap), c->P);
    g->chunks = (c->P + g->rows - 1) / g->rows;
    if (g->chunks > 65535u) { set_error("%s cuts the rows into more than 65,535 chunks", rows_switch); return MK_ERR_ARG; }
    return MK_OK;
}

template <class Table, class Acc>
void launch_table_pass(mk_ctx *c, const PassGrid &g, const typename Table::Cell *d_table, const Acc &acc)
{
    const dim3 grid(g.columns, g.chunks), block(256);
    if (c->W == 1) hipLaunchKernelGGL((table_pass_kernel<1, Table, Acc>), grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, c->G, g.ntiles, g.rows, d_table, acc);
    else hipLaunchKernelGGL((table_pass_kernel<2, Table, Acc>), grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, c->G, g.ntiles, g.rows, d_table, acc);
}

}  // namespace

}  // namespace mk
