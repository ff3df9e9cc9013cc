// K6h: depth of coverage -- per indexed genome, how often the reads of a set hold each of its stored fingerprints, and the
// median of that over the fingerprints they hold at all (Mash screen's median multiplicity).
//
// For a set of queries Q (a multiset: a query given twice counts twice):
//   mult(p, v)   min(255, #{ q in Q : the GATED sketch of q (minhash_sketch_partition_solid_kmers, Miekki.cpp:214-224) has value
//                v != empty at partition p }); MK_DEPTH_MAX = 255
//   covered(g)   #{ p : column_g[p] != empty and mult(p, column_g[p]) > 0 } -- mk_cover_count's covered for the same queries
//   sum(g)       the sum of mult(p, column_g[p]) over those p, 64 bits; the mean depth is sum / covered, which the caller divides
//   median(g)    the LOWER median of those covered(g) values: sorted ascending, the element of index (covered - 1) / 2; equally
//                the largest t in 1..255 with #{ p : column_g[p] != empty, mult(p, column_g[p]) >= t } >= covered(g) / 2 + 1;
//                0 when covered(g) = 0
//   cells        #{ (p, v) : mult > 0 }
//   saturated    #{ (p, v) : mult = 255 }
// Passes ACCUMULATE with saturation: a pass made twice doubles the multiplicities up to the cap.  min(255, count) does not depend
// on the order of the increments, so the result is a function of the multiset of queries and the matrix and of nothing else.
// Integers only, no thresholds.  A median of 255 means "255 or more": `saturated` is reported for that reason.  With 8-bit
// fingerprints read `median` only where covered / sketch_size stands clear of the floor cells / (P * 256).
//
// `mult` is a table of one byte per (partition, fingerprint value) in caller-owned device memory: byte (p << fp_bits) + v,
// P << fp_bits bytes.
//
//   mark:    cover.hip's walks (one wave per sparse query over its entry list; one lane per (group, partition) of the dense
//            slots, empty slots skipped), the mark a saturating byte increment.  There is no byte atomic: a compare-and-swap loop
//            on the containing dword, agent scope, relaxed, adds 1 to the one byte, leaves the other three as they are read, and
//            stops when the byte reads 255.  (Not an add with an undo after overflow: between the two a wrapped byte reads 0 to a
//            third lane, which would add to it.)  FILTER: the loop's first expected value comes from a plain load; a byte that
//            reads 255 there cannot be stale -- counters never fall inside a pass -- and no atomic is issued; a stale smaller
//            value costs one failed compare-and-swap, which returns the fresh dword, never a wrong count.  Without the filter
//            the first expected value is 0 and the first compare-and-swap fetches the dword.
//   profile: the count pass's shape (cover.hip) with a byte lookup: a workgroup owns 4 x T tiles of 1 KiB (16 bytes per lane)
//            and a chunk of rows, counts in 32-bit registers, the next rows' loads in flight while a group of rows is looked up;
//            hot and cold rows alike through mat_row; genomes g < G only; `empty` never counts.  One byte: the table goes
//            through LDS 8 KiB at a time, double buffered -- the 256-byte slices of 32 rows, the slice's last byte (`empty`'s)
//            zeroed on the way in -- and a lane reads one LDS byte per fingerprint.  Two bytes: a row's slice is 64 KiB and the
//            bytes are looked up where they lie, through L1 / L2, `empty` skipped by value.
//            Pass 0: per lane covered += m > 0 and sum += m (a chunk has at most 2^24 rows: 255 * rows fits 32 bits), then one
//            relaxed agent-scope add per genome and chunk for each (sum: 64 bits).
//            Passes 1..8: the median by bisection on t, no histogram.  lo = 1, hi = 255 per genome in device memory; a step
//            takes mid = (lo + hi + 1) / 2, a pass counts m >= mid[g] (a lane reads its genomes' mid once), and a small kernel
//            sets lo = mid where the count is at least covered / 2 + 1, else hi = mid - 1.  After 8 steps median = covered ? lo
//            : 0.  All 8 steps run whatever the data; nothing waits on the host in between.
//   cells:   a reduction over the table: its non-zero bytes and its bytes of 255.
#include <algorithm>
#include <cstdlib>

#include "mk_internal.hpp"

namespace mk {

namespace {

// one more for the byte at `cell`, up to 255
template <bool FILTER>
__device__ __forceinline__ void bump(uint8_t *__restrict__ mult, uint64_t cell)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(mult + (cell & ~3ull));
    const uint32_t shift = ((uint32_t)cell & 3u) * 8u;
    uint32_t old = FILTER ? *w : 0u;
    for (;;) {
        if (((old >> shift) & 255u) == 255u) return;
        // (a failure leaves the dword as it is and the fresh value in `old`)
        if (__hip_atomic_compare_exchange_strong(w, &old, old + (1u << shift), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

template <bool FILTER>
__global__ __launch_bounds__(256) void depth_mark_sparse_kernel(const uint64_t *__restrict__ entries, const uint64_t *__restrict__ ent_off,
                                                                const uint32_t *__restrict__ scan_n, uint32_t nq, uint32_t P, uint32_t fp_bits,
                                                                uint32_t empty, uint8_t *__restrict__ mult)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (q >= nq) return;
    const uint32_t n = scan_n[q];                                          // (0 for the dense queries: their slots are walked below)
    const uint64_t *__restrict__ e = entries + ent_off[q];
    for (uint32_t i = lane; i < n; i += 64u) {
        const uint64_t ent = e[i];
        const uint32_t p = (uint32_t)ent, v = (uint32_t)(ent >> 32);
        if (p < P && v < empty) bump<FILTER>(mult, ((uint64_t)p << fp_bits) + v);
    }
}

template <int W, bool FILTER>
__global__ __launch_bounds__(256) void depth_mark_dense_kernel(const uint8_t *__restrict__ dense, uint64_t n, uint32_t P, uint8_t *__restrict__ mult)
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
        if (v != kEmpty) bump<FILTER>(mult, ((uint64_t)p << kBits) + v);
    }
}

constexpr uint32_t kStageVec = 512;       // one byte: the table goes through LDS 8 KiB at a time, the slices of 32 rows
constexpr uint32_t kSliceVec = 16;        // uint4s of one row's slice at one byte

template <int W> struct DepthShape;
template <> struct DepthShape<1> { static constexpr uint32_t T = 1, RU = 8; };   // tiles per wave, rows in flight per wave
template <> struct DepthShape<2> { static constexpr uint32_t T = 4, RU = 1; };

// BISECT false: pass 0, count[g] += #{ m > 0 }, sum[g] += m.  BISECT true: count[g] += #{ m >= mid[g] } (mid >= 1).
template <int W, bool BISECT>
__global__ __launch_bounds__(256) void depth_pass_kernel(MatRef M, uint64_t ld, uint32_t P, uint32_t G, uint32_t ntiles, uint32_t rows_per_chunk,
                                                         const uint8_t *__restrict__ mult, const uint32_t *__restrict__ mid,
                                                         uint32_t *__restrict__ count, unsigned long long *__restrict__ sum)
{
    constexpr uint32_t T = DepthShape<W>::T, RU = DepthShape<W>::RU;
    constexpr uint32_t kBits = 8 * W, kMask = (1u << kBits) - 1u, kPerLane = 16u / W;
    constexpr uint32_t kStageRows = kStageVec / kSliceVec;
    static_assert(kStageRows % RU == 0, "a group of rows lies in one stage");
    __shared__ uint4 s_tab[W == 1 ? 2 : 1][W == 1 ? kStageVec : 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tile0 = (blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(tid >> 6)) * T;
    const uint32_t r_lo = blockIdx.y * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);          // (rows_per_chunk <= P <= 2^28)
    const uint32_t nrows = r_hi - r_lo, ngroups = (nrows + RU - 1) / RU, nstages = (nrows + kStageRows - 1) / kStageRows;
    const uint64_t tab_vec = (uint64_t)P * kSliceVec;
    const uint4 *__restrict__ mult4 = reinterpret_cast<const uint4 *>(mult);

    uint4 tv[2];
    auto fetch = [&](uint32_t s) {
        const uint64_t base = ((uint64_t)r_lo + (uint64_t)s * kStageRows) * kSliceVec;
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint64_t idx = base + tid + 256u * u;
            tv[u] = idx < tab_vec ? mult4[idx] : make_uint4(0, 0, 0, 0);   // (a stage may reach past the chunk, never past the table)
        }
    };
    auto put = [&](uint32_t b) {
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            const uint32_t j = tid + 256u * u;
            uint4 x = tv[u];
            if ((j & (kSliceVec - 1u)) == kSliceVec - 1u) x.w &= 0x00ffffffu;   // the slice's last byte is `empty`'s
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
    uint32_t cnt[T][kPerLane], acc[T][kPerLane], thr[T][kPerLane];
#pragma unroll
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t g0 = (tile0 + t) * (kTileBytes / W) + lane * kPerLane;
#pragma unroll
        for (uint32_t j = 0; j < kPerLane; ++j) {
            cnt[t][j] = 0;
            acc[t][j] = 0;
            thr[t][j] = BISECT && g0 + j < G ? mid[g0 + j] : 1u;
        }
    }

    if (W == 1) {
        fetch(0);
        put(0);
    }
    load(0, cur);
    if (W == 1) __syncthreads();
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t row = g * RU, s = row / kStageRows;                 // the group's first row in the chunk, its stage
        const bool first = row % kStageRows == 0, last = (row + RU) % kStageRows == 0 || g + 1 == ngroups;
        if (W == 1 && first && s + 1 < nstages) fetch(s + 1);
        if (g + 1 < ngroups) load(g + 1, nxt);
        const uint8_t *tab = reinterpret_cast<const uint8_t *>(s_tab[W == 1 ? s & 1u : 0u]) + (row - s * kStageRows) * (kSliceVec * 16u);
#pragma unroll
        for (uint32_t u = 0; u < RU; ++u) {
            if (row + u >= nrows) break;                                   // (uniform)
            const uint8_t *sl = W == 1 ? tab + u * (kSliceVec * 16u) : mult + ((uint64_t)(r_lo + row + u) << kBits);
#pragma unroll
            for (uint32_t t = 0; t < T; ++t) {
                if (tile0 + t >= ntiles) continue;
                const uint32_t w[4] = {cur[u][t].x, cur[u][t].y, cur[u][t].z, cur[u][t].w};
#pragma unroll
                for (uint32_t j = 0; j < kPerLane; ++j) {
                    const uint32_t v = (w[j * W / 4] >> ((j * kBits) & 31u)) & kMask;
                    const uint32_t m = W == 2 && v == kMask ? 0u : sl[v];  // (one byte: the staged slice holds 0 at `empty`)
                    cnt[t][j] += m >= thr[t][j];
                    if (!BISECT) acc[t][j] += m;
                }
            }
        }
        if (W == 1) {
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
        for (uint32_t j = 0; j < kPerLane; ++j) {
            if (g0 + j >= G || !cnt[t][j]) continue;                               // (columns [G, pitch) are zero padding)
            (void)__hip_atomic_fetch_add(count + g0 + j, cnt[t][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!BISECT) (void)__hip_atomic_fetch_add(sum + g0 + j, (unsigned long long)acc[t][j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// One step of the bisection for every genome.  step 0: lo = 1, hi = 255.  step k > 0: the pass before counted m >= mid into
// count[g], which is read and zeroed for the next pass.  After `steps` steps: out[g] = { sum, covered, covered ? lo : 0 }.
__global__ __launch_bounds__(256) void depth_step_kernel(uint32_t G, uint32_t step, uint32_t steps, const uint32_t *__restrict__ covered,
                                                         const unsigned long long *__restrict__ sum, uint32_t *__restrict__ count,
                                                         uint32_t *__restrict__ lo, uint32_t *__restrict__ hi, uint32_t *__restrict__ mid,
                                                         mk_depth *__restrict__ out)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= G) return;
    const uint32_t cov = covered[g];
    uint32_t l = 1u, h = MK_DEPTH_MAX;
    if (step) {
        l = lo[g];
        h = hi[g];
        const uint32_t m = mid[g];
        if (count[g] >= cov / 2u + 1u) l = m; else h = m - 1u;             // (lo's count is at least that throughout: hi >= lo)
        count[g] = 0;
    }
    lo[g] = l;
    hi[g] = h;
    mid[g] = (l + h + 1u) / 2u;
    if (step == steps) {
        mk_depth d;
        d.sum = sum[g];
        d.covered = cov;
        d.median = cov ? l : 0u;
        out[g] = d;
    }
}

// bytes of x that are not zero, as a count
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x)
{
    return __popc((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u);
}

// totals[0] += the table's non-zero bytes, totals[1] += its bytes of 255
__global__ __launch_bounds__(256) void depth_cells_kernel(const uint4 *__restrict__ mult4, uint64_t nvec, unsigned long long *__restrict__ totals)
{
    uint32_t n = 0, f = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < nvec; i += (uint64_t)gridDim.x * 256u) {
        const uint4 x = mult4[i];
        // (a lane's share stays far below 2^32: at most 2^44 bytes over 2^19 lanes)
        n += nonzero_bytes(x.x) + nonzero_bytes(x.y) + nonzero_bytes(x.z) + nonzero_bytes(x.w);
        f += 16u - (nonzero_bytes(~x.x) + nonzero_bytes(~x.y) + nonzero_bytes(~x.z) + nonzero_bytes(~x.w));
    }
    uint64_t cells = n, full = f;
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) {
        cells += __shfl_xor(cells, o);
        full += __shfl_xor(full, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (cells) (void)__hip_atomic_fetch_add(totals, (unsigned long long)cells, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (full) (void)__hip_atomic_fetch_add(totals + 1, (unsigned long long)full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

uint64_t depth_table_bytes(const mk_ctx *c) { return (uint64_t)c->P << c->p.fp_bits; }

int launch_depth_reset(mk_ctx *c, uint8_t *d_mult)
{
    MK_HIP(hipMemsetAsync(d_mult, 0, depth_table_bytes(c), c->stream));
    return MK_OK;
}

// MIEKKI_DEPTH_FILTER=0 / 1: the marks without / with the plain load in front of the compare-and-swap (tools/depth_rate.py
// measures both)
static bool depth_filter()
{
    if (const char *e = getenv("MIEKKI_DEPTH_FILTER")) return atol(e) != 0;
    return true;
}

int launch_depth_mark(mk_ctx *c, const mk_qset *qs, uint8_t *d_mult)
{
    if (!qs->nq) return MK_OK;
    const bool filter = depth_filter();
    if (!qs->columns) {
        const dim3 grid((qs->nq + 3) / 4), block(256);
        if (filter) hipLaunchKernelGGL(depth_mark_sparse_kernel<true>, grid, block, 0, c->stream, qs->d_entries, qs->d_ent_off, qs->d_scan_n, qs->nq, c->P, c->p.fp_bits, c->empty, d_mult);
        else hipLaunchKernelGGL(depth_mark_sparse_kernel<false>, grid, block, 0, c->stream, qs->d_entries, qs->d_ent_off, qs->d_scan_n, qs->nq, c->P, c->p.fp_bits, c->empty, d_mult);
    }
    if (!qs->dense_q.empty()) {
        const uint64_t n = (uint64_t)(qs->dense_q.size() / 4) * c->P, blocks = (n + 255) / 256;
        if (blocks > 0x7fffffffull) { set_error("too many dense queries for one mark pass"); return MK_ERR_ARG; }
        const dim3 grid((uint32_t)blocks), block(256);
        if (c->W == 1) {
            if (filter) hipLaunchKernelGGL((depth_mark_dense_kernel<1, true>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_mult);
            else hipLaunchKernelGGL((depth_mark_dense_kernel<1, false>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_mult);
        } else {
            if (filter) hipLaunchKernelGGL((depth_mark_dense_kernel<2, true>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_mult);
            else hipLaunchKernelGGL((depth_mark_dense_kernel<2, false>), grid, block, 0, c->stream, qs->d_dense, n, c->P, d_mult);
        }
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// Rows per chunk, as the count pass chooses them: enough workgroups to fill the device several times over (2,048), whole stages
// of the table, at least 256 (64) rows so that a genome's adds at the end of a chunk stand against 256 (128) bytes read -- and
// at most 2^24, so that a lane's sum of bytes fits 32 bits.  MIEKKI_DEPTH_ROWS: the tests make small indexes take several
// chunks, whole stages or not.
static uint32_t depth_rows_per_chunk(const mk_ctx *c, uint32_t columns)
{
    const uint32_t stage_rows = c->W == 1 ? kStageVec / kSliceVec : 1u, least = c->W == 1 ? 256u : 64u;
    const uint64_t chunks = std::max<uint64_t>(1, 2048 / columns);
    uint64_t rows = std::max<uint64_t>(least, (c->P + chunks - 1) / chunks);
    rows = (rows + stage_rows - 1) / stage_rows * stage_rows;
    if (const char *e = getenv("MIEKKI_DEPTH_ROWS")) { const long v = atol(e); if (v >= 1) rows = (uint64_t)v; }
    return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(rows, 1u << 24), c->P);
}

// MIEKKI_DEPTH_STEPS=0..8: a measurement switch (tools/depth_rate.py): the bisection stops after so many steps, and `median` is
// then the lower end of an interval that is not closed.  8 unless set.
static uint32_t depth_steps()
{
    if (const char *e = getenv("MIEKKI_DEPTH_STEPS")) { const long v = atol(e); if (v >= 0 && v < 8) return (uint32_t)v; }
    return 8;
}

uint64_t depth_scratch_words(uint32_t G) { return (uint64_t)G * 7; }

// d_out[G] is written; d_scratch: depth_scratch_words(G) 32-bit words at an 8-byte boundary; raw cold rows
int launch_depth_profile(mk_ctx *c, const uint8_t *d_mult, uint32_t *d_scratch, mk_depth *d_out)
{
    const uint32_t G = c->G;
    if (!G) return MK_OK;
    const uint32_t ntiles = (uint32_t)(((uint64_t)G * c->W + kTileBytes - 1) / kTileBytes);
    if ((uint64_t)ntiles * kTileBytes > c->ld) { set_error("the matrix rows do not cover whole tiles"); return MK_ERR_STATE; }
    const uint32_t per_wg = 4u * (c->W == 1 ? DepthShape<1>::T : DepthShape<2>::T), columns = (ntiles + per_wg - 1) / per_wg;
    const uint32_t rows = depth_rows_per_chunk(c, columns), chunks = (c->P + rows - 1) / rows, steps = depth_steps();
    if (chunks > 65535u) { set_error("MIEKKI_DEPTH_ROWS cuts the rows into more than 65,535 chunks"); return MK_ERR_ARG; }
    // [sum: G x 8 bytes][covered: G][count: G][lo: G][hi: G][mid: G]
    unsigned long long *d_sum = reinterpret_cast<unsigned long long *>(d_scratch);
    uint32_t *d_cov = d_scratch + (size_t)G * 2, *d_cnt = d_cov + G, *d_lo = d_cnt + G, *d_hi = d_lo + G, *d_mid = d_hi + G;
    MK_HIP(hipMemsetAsync(d_scratch, 0, (size_t)G * 16, c->stream));       // sum, covered, count
    const dim3 grid(columns, chunks), block(256), sgrid((G + 255) / 256);
    const MatRef M = mat_ref(c);
    if (c->W == 1) hipLaunchKernelGGL((depth_pass_kernel<1, false>), grid, block, 0, c->stream, M, c->ld, c->P, G, ntiles, rows, d_mult, (const uint32_t *)nullptr, d_cov, d_sum);
    else hipLaunchKernelGGL((depth_pass_kernel<2, false>), grid, block, 0, c->stream, M, c->ld, c->P, G, ntiles, rows, d_mult, (const uint32_t *)nullptr, d_cov, d_sum);
    for (uint32_t step = 0;; ++step) {
        hipLaunchKernelGGL(depth_step_kernel, sgrid, block, 0, c->stream, G, step, steps, d_cov, d_sum, d_cnt, d_lo, d_hi, d_mid, d_out);
        if (step == steps) break;
        if (c->W == 1) hipLaunchKernelGGL((depth_pass_kernel<1, true>), grid, block, 0, c->stream, M, c->ld, c->P, G, ntiles, rows, d_mult, d_mid, d_cnt, (unsigned long long *)nullptr);
        else hipLaunchKernelGGL((depth_pass_kernel<2, true>), grid, block, 0, c->stream, M, c->ld, c->P, G, ntiles, rows, d_mult, d_mid, d_cnt, (unsigned long long *)nullptr);
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// d_totals[0] (cells) and d_totals[1] (saturated) are ADDED to: the caller zeroes them
int launch_depth_cells(mk_ctx *c, const uint8_t *d_mult, unsigned long long *d_totals)
{
    const uint64_t nvec = depth_table_bytes(c) / 16;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(2048, (nvec + 255) / 256);
    hipLaunchKernelGGL(depth_cells_kernel, dim3(blocks), dim3(256), 0, c->stream, reinterpret_cast<const uint4 *>(d_mult), nvec, d_totals);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
