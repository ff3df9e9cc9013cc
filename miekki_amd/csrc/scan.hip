// K5: query-vs-all-genomes fingerprint scan -- launchers.  The kernels are in
// scan_kernel.hpp (shared with tools/scan_tune.hip); DESIGN.md section 4.1 has the
// measurements behind each choice.  Every launcher sizes its grid with launch_grid and
// picks the kernel's template arguments with pick; which kernel walks a set's partition
// ranges is SlabArgs::kind, chosen when the set is prepared (api_query.hip, qset_prepare_slab).
//
// Replaces the loop nest of Miekki::query_sequences (Miekki.cpp:355-369); the
// filter of Miekki::filter_results runs over the scores in select.hip (K6).
//
// One WAVE owns one (query, 1 KiB row tile) pair -- 1024 genomes at 1-byte
// fingerprints, 512 at 2-byte -- so that tiny collections (G = 1000 is one tile) and
// huge ones (G = 100,000 is 98 tiles) both fill the 256 CUs.  The query's sparse
// sketch is wave-uniform: it is staged in SGPRs through the scalar cache, the row base
// is scalar arithmetic, and every lane issues one 16-byte load per entry from
// M[p][tile*1024 + lane*16].  Fingerprints are compared four (two) at a time with
// SWAR zero-byte detection on the XOR against the broadcast query fingerprint, into
// packed 8-bit (16-bit) per-genome counters.  A pure row stream (no atomics, no LDS but in
// scan_block_kernel) whose speed is decided by the ORDER of the work items and by how often
// a row piece is fetched:
//   scan_block_kernel  (tile, partition range, block of queries, 128-byte sub-tile): a workgroup
//                      counts a block of 1,280 queries in LDS (64-bit integer adds) from a list grouped
//                      by partition, so a row piece is loaded once for all the block's queries
//                      that want it -- sets with a range table and at least a block of queries; within a
//                      (tile, range) the work items run block fastest (SlabArgs::block_sub_fast = 1), so
//                      the workgroups in flight on an XCD are up to 32 blocks on ONE sub-tile and find
//                      each other's row pieces in L2 (hit rate 0.79 against 0.32 sub-tile fastest);
//   scan_group_kernel  (tile, partition range, group of queries): a wave carries a group's
//                      counters and walks its merged list window by window, so the waves
//                      in flight on an XCD share row pieces through L2 -- smaller sets with a
//                      range table;
//   scan_slab_kernel   (tile, partition range, query): the waves in flight share a
//                      128 MiB slab that the Infinity Cache holds -- small sets (ranges by
//                      count) and cold rows read in place;
//   scan_kernel        tile-major over whole entry lists, u32 scores -- long queries,
//                      score export;
//   scan_dense_kernel  four whole-genome queries per pass over the matrix (-A).
#include <algorithm>

#include "scan_kernel.hpp"

namespace mk {

// f(std::integral_constant<int, V>) for the V among Vs that v equals (the last of them for any other v): a run-time
// number -- the fingerprint width, queries per wave -- picks a kernel's template argument
template <int V, int... Vs, typename F>
static auto pick(int v, F f)
{
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V>{});
    else if (v == V) return f(std::integral_constant<int, V>{});
    else return pick<Vs...>(v, f);
}

// the grid of a launch of `work` items, per_wg to a workgroup; dealt: a multiple of eight workgroups, for a kernel that
// deals them to the XCDs (xcd_workgroup).  0: nothing to do.
static int launch_grid(uint64_t work, uint32_t per_wg, bool dealt, const char *what, uint32_t *blocks)
{
    if (work >= (1ull << 31)) { set_error("%s launch too large", what); return MK_ERR_ARG; }
    const uint32_t wgs = (uint32_t)((work + per_wg - 1) / per_wg);
    *blocks = dealt ? xcd_grid(wgs) : wgs;
    return MK_OK;
}

int launch_scan(mk_ctx *c, const ScanArgs &a)
{
    uint32_t blocks;
    MK_TRY(launch_grid((uint64_t)a.nq * a.ntiles, 4, false, "scan", &blocks));
    if (!blocks) return MK_OK;
    pick<1, 2>(c->W, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if (a.windowed) hipLaunchKernelGGL((scan_kernel<W, 8, 1, false, true>), dim3(blocks), dim3(256), 0, c->stream, a);
        else            hipLaunchKernelGGL((scan_kernel<W, 8, 1, false, false>), dim3(blocks), dim3(256), 0, c->stream, a);
    });
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_scan_slab(mk_ctx *c, const SlabArgs &a)
{
    if (a.nq == 0) return MK_OK;
    const uint64_t tr = (uint64_t)a.ntiles * a.r_count;                // (tile, range) pairs of the launch
    // the first and last group / block of the set's that the launch's queries touch, and those between
    auto spanned = [&](uint32_t per) { return (uint64_t)((a.q_begin + a.nq - 1) / per - a.q_begin / per + 1); };
    uint32_t blocks;
    switch (a.kind) {
    case RangedScan::Blocks: {
        if (a.block_q == 0 || a.block_q > kBlockQ) { set_error("scan blocks of %u queries", a.block_q); return MK_ERR_ARG; }
        // (the work order: whole runs of sub-tiles, or the kernel's decode would name sub-tiles a tile does not have)
        if (a.block_sub_fast != 1 && a.block_sub_fast != 2 && a.block_sub_fast != 4 && a.block_sub_fast != 8) {
            set_error("scan blocks: %u sub-tiles fastest (1, 2, 4 or 8)", a.block_sub_fast);
            return MK_ERR_ARG;
        }
        static_assert(kTileBytes / kBlockTile == 8, "the orders launch_scan_slab lets through divide a tile's sub-tiles");
        // (the kernel reaches a row by one 32 x 32-bit multiply-add of its place in the range and the pitch: piece_base)
        if (a.ld >> 32) { set_error("scan blocks: a row pitch of %llu bytes", (unsigned long long)a.ld); return MK_ERR_ARG; }
        // ... from the range's first row in ONE home, chosen per workgroup: the range P_hot falls into is not for this
        // kernel where it lies (qset_scan_slab stages it in HBM as a whole)
        if (a.Mc && a.Mc != a.M && a.range_rows) {
            const uint32_t rc = std::min(a.P_hot / a.range_rows, a.S - 1);      // the range of the first cold row
            if (rc >= a.r_begin && rc - a.r_begin < a.r_count && a.P_hot > rc * a.range_rows) {
                set_error("scan blocks: range %u has rows on both sides of row %u", rc, a.P_hot);
                return MK_ERR_ARG;
            }
        }
        MK_TRY(launch_grid(tr * spanned(a.block_q) * (kTileBytes / kBlockTile), 1, true, "scan", &blocks));
        if (!blocks) return MK_OK;
        // scan_block_kernel's LDS: a block's counters, beyond the 64 KiB a kernel has without asking -- up to all 160 KiB of a
        // CU (the kernel has no static LDS)
        const uint32_t lds = std::max<uint32_t>(a.block_q * kBlockTile, 16u);
        return pick<1, 2>(c->W, [&](auto w) -> int {
            constexpr int W = decltype(w)::value;
            // (asked for at every launch: the attribute belongs to the device the context is bound to, and a process may hold several)
            MK_HIP(hipFuncSetAttribute((const void *)scan_block_kernel<W, kBlockTile>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kBlockQ * kBlockTile)));
            // (four packets and rows in flight per lane group; eight measured slower, profiles/r8_scan_blocks_ab.txt)
            hipLaunchKernelGGL((scan_block_kernel<W, kBlockTile>), dim3(blocks), dim3(1024), lds, c->stream, a);
            MK_HIP(hipGetLastError());
            return MK_OK;
        });
    }
    case RangedScan::Groups:
        MK_TRY(launch_grid(tr * spanned(kGroupQ), 4, true, "scan", &blocks));
        if (!blocks) return MK_OK;
        // (four 16-byte loads in flight per wave: registers hold the group's 16 x 4 counters besides)
        pick<1, 2>(c->W, [&](auto w) { hipLaunchKernelGGL((scan_group_kernel<decltype(w)::value, kGroupQ, 4>), dim3(blocks), dim3(256), 0, c->stream, a); });
        break;
    case RangedScan::ByCount:
    case RangedScan::PerWave:
        MK_TRY(launch_grid(tr * a.nq, 4, false, "scan", &blocks));
        if (!blocks) return MK_OK;
        pick<1, 2>(c->W, [&](auto w) { hipLaunchKernelGGL((scan_slab_kernel<decltype(w)::value, 8>), dim3(blocks), dim3(256), 0, c->stream, a); });
        break;
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// the groups' merged lists of a set (every range of its range table): one workgroup per (group, range)
int launch_group_lists(mk_ctx *c, mk_qset *qs, uint32_t wshift, uint32_t nwin)
{
    if (!qs->nq) return MK_OK;
    GroupArgs a;
    a.entries = qs->d_entries; a.ent_off = qs->d_ent_off; a.split = qs->d_split; a.lists = qs->d_glist;
    a.nq = qs->nq; a.S = qs->S; a.P = c->P; a.wshift = wshift; a.nwin = nwin;
    const dim3 grid((qs->nq + kGroupQ - 1) / kGroupQ, qs->S);
    hipLaunchKernelGGL(group_list_kernel<kGroupQ>, grid, dim3(256), 0, c->stream, a);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// the blocks' lists of a set (every range of its range table): one workgroup per (block, range)
int launch_block_lists(mk_ctx *c, mk_qset *qs)
{
    if (!qs->nq) return MK_OK;
    BlockListArgs a;
    a.entries = qs->d_entries; a.ent_off = qs->d_ent_off; a.split = qs->d_split;
    a.packets = qs->d_bpackets; a.info = qs->d_binfo;
    a.nq = qs->nq; a.S = qs->S; a.P = c->P; a.B = qs->block_q;
    a.W = c->W; a.pitch = kBlockTile;                                   // (what scan_block_kernel<W, kBlockTile> takes a pair word for)
    const dim3 grid((qs->nq + qs->block_q - 1) / qs->block_q, qs->S);
    hipLaunchKernelGGL(block_list_kernel, grid, dim3(1024), 0, c->stream, a);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_dense_lut(mk_ctx *c, const uint8_t *d_dense, uint32_t ngroups, DenseLut *d_lut)
{
    if (!ngroups) return MK_OK;
    pick<1, 2>(c->W, [&](auto w) {
        hipLaunchKernelGGL(dense_lut_kernel<decltype(w)::value>, dim3((c->P + 255) / 256, (ngroups + 1) / 2), dim3(256), 0, c->stream, d_dense, ngroups, c->P, c->empty, d_lut);
    });
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_scan_dense(mk_ctx *c, const DenseArgs &a)
{
    uint32_t blocks;
    // by table, sixteen queries per pass over the matrix (eight when there are no more)
    // (the table kernel walks rows in groups of sixteen: every window and chunk of rows is a multiple of that for P >= 16;
    // sketches of fewer partitions take the compare kernel below)
    if (a.lut && a.rows_per_item % 16 == 0 && (a.row_hi - a.row_lo) % 16 == 0) {
        // (sixteen queries per wave: eight -- a third more instructions per query for a third wave per SIMD -- measured 97 against
        // 79 ms at 64 queries, profiles/r6_pmc_dense.txt)
        const uint32_t no = a.noctets >= 2 ? 2 : 1;
        // the sets of sixteen (eight) queries share a tile's rows through LDS, two or four waves of a workgroup (scan_kernel.hpp)
        const uint32_t nsets = (a.noctets + no - 1) / no, gs = dense_share(a.noctets);
        MK_TRY(launch_grid((uint64_t)((nsets + gs - 1) / gs) * a.ntiles * a.nchunks, 4 / gs, true, "dense scan", &blocks));
        if (!blocks) return MK_OK;
        pick<1, 2>(c->W, [&](auto w) { pick<1, 2>(no, [&](auto o) { pick<1, 2, 4>(gs, [&](auto g) {
            hipLaunchKernelGGL((scan_dense_lut_kernel<decltype(w)::value, decltype(o)::value, decltype(g)::value>), dim3(blocks), dim3(256), 0, c->stream, a);
        }); }); });
        MK_HIP(hipGetLastError());
        return MK_OK;
    }
    // eight queries per pass over the matrix when there are that many, else four
    const uint32_t gb = a.ngroups >= 2 ? 2 : 1;
    MK_TRY(launch_grid((uint64_t)((a.ngroups + gb - 1) / gb) * a.ntiles * a.nchunks, 4, false, "dense scan", &blocks));
    if (!blocks) return MK_OK;
    pick<1, 2>(c->W, [&](auto w) { pick<1, 2>(gb, [&](auto g) {
        hipLaunchKernelGGL((scan_dense_kernel<decltype(w)::value, decltype(g)::value>), dim3(blocks), dim3(256), 0, c->stream, a);
    }); });
    MK_HIP(hipGetLastError());
    return MK_OK;
}

// ---- the box's read-only stream ceiling (SURVEY.md 8d asks for it next to the spec peak):
// every lane sums 16-byte loads over the resident matrix buffer, grid-stride, eight loads in
// flight.  Measurement aid behind mk_probe_stream_read; nothing on the query path calls it.
__global__ __launch_bounds__(256) void stream_read_kernel(const uint4 *__restrict__ p, uint64_t n16, uint32_t *sink)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t acc = 0;
    for (; i + 7 * stride < n16; i += 8 * stride) {
        uint4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[i + u * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    for (; i < n16; i += stride) { const uint4 v = p[i]; acc += v.x ^ v.y ^ v.z ^ v.w; }
    if (acc == 0x12345678u) *sink = acc;                       // keeps the loads live
}

int probe_stream_read(mk_ctx *c, uint32_t rounds, double *gbps, uint64_t *bytes)
{
    const uint64_t total = (uint64_t)c->P_hot * c->ld;             // the rows resident in HBM
    *gbps = 0; *bytes = total;
    if (!c->d_M || total < (1ull << 20)) return MK_OK;
    if (!c->d_flag) MK_TRY(c->d_flag.alloc(1));
    hipEvent_t e0, e1;
    MK_HIP(hipEventCreate(&e0)); MK_HIP(hipEventCreate(&e1));
    float best = 0;
    for (uint32_t r = 0; r <= rounds; ++r) {                    // first round warms up
        MK_HIP(hipEventRecord(e0, c->stream));
        hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 8), dim3(256), 0, c->stream, (const uint4 *)c->d_M, total / 16,
                           c->d_flag);
        MK_HIP(hipEventRecord(e1, c->stream));
        MK_HIP(hipEventSynchronize(e1));
        float ms = 0;
        MK_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (r && (best == 0 || ms < best)) best = ms;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (best > 0) *gbps = (double)total / best / 1e6;
    return MK_OK;
}

// ---- scan_block_kernel's compare on its own: flags[i] = ne_lanes_block(d[i], b[i]) .
// Test aid behind mk_probe_ne_lanes; nothing on the query path calls it.
template <int W>
__global__ __launch_bounds__(256) void ne_lanes_probe_kernel(const uint32_t *__restrict__ d, const uint32_t *__restrict__ b, uint64_t n,
                                                             uint32_t *__restrict__ flags)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = ne_lanes_block<W>(d[i], b[i]);
}

int probe_ne_lanes(mk_ctx *c, uint32_t W, const uint32_t *d, const uint32_t *b, uint64_t n, uint32_t *flags)
{
    if (!n) return MK_OK;
    uint32_t *dd = nullptr, *db = nullptr, *df = nullptr;
    int rc = dev_alloc(&dd, n);
    if (rc == MK_OK) rc = dev_alloc(&db, n);
    if (rc == MK_OK) rc = dev_alloc(&df, n);
    if (rc == MK_OK && (hipMemcpyAsync(dd, d, n * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                        hipMemcpyAsync(db, b, n * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess)) rc = MK_ERR_DEVICE;
    if (rc == MK_OK) {
        const dim3 grid((uint32_t)((n + 255) / 256));
        if (W == 1) hipLaunchKernelGGL(ne_lanes_probe_kernel<1>, grid, dim3(256), 0, c->stream, dd, db, n, df);
        else        hipLaunchKernelGGL(ne_lanes_probe_kernel<2>, grid, dim3(256), 0, c->stream, dd, db, n, df);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(flags, df, n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) rc = MK_ERR_DEVICE;
    }
    if (rc == MK_ERR_DEVICE) set_error("compare probe failed");
    dev_free(dd); dev_free(db); dev_free(df);
    return rc;
}

}  // namespace mk
