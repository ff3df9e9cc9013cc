// mk_index_select: keep the genomes ids[0 .. n) of the index, in that order, in place.  The matrix is partition-major and a
// row holds W bytes per genome, so the operation is the same gather inside every row: new row[j] = old row[ids[j]].  The
// rows never leave the device (cold rows: never leave the host memory they live in, addressed through mat_row).
//
// A row cannot be gathered onto itself, so the rows go in blocks through the context's column staging buffer (d_colstage):
//   1. keep_gather_kernel: stage[r][j] = row[p0 + r][ids[j]], 16 bytes per lane, a wave per 1 KiB PIECE of a new row;
//   2. keep_store_kernel:  the stage back to the front of the same rows and zeros behind it up to the old width, 16 bytes
//      per lane -- columns [n, old G) are zero afterwards, which is what ensure_capacity hands a later append.
// The leading columns that stay where they are (ids[j] == j) are not touched by either: whole pieces of them are skipped, so
// dropping the last genome of 100,000 moves one piece per row.
//
// Where a lane's 16 bytes come from is chosen per piece on the host, as colq.hip chooses per 64 slots:
//   - an ASCENDING piece whose sources lie within kKeepSpan bytes of the row (what removing genomes produces: a subset in
//     index order): the wave loads that span with 16-byte loads into LDS and picks its bytes there;
//   - any other piece (a permutation): a byte (W = 2: halfword) load per output element straight from the row, which is
//     100 KB at 100,000 genomes and stays in L2 while the row's pieces are made.
// The ids are padded to whole pieces and come with 16-byte loads.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "mk_internal.hpp"

namespace mk {

constexpr uint32_t kKeepPiece = 1024;    // bytes of a new row one wave makes: 64 lanes x 16 B
constexpr uint32_t kKeepSpan = 4096;     // most source bytes (whole 16-byte chunks) a piece takes through LDS

// span path: the piece's sources lie in chunks [chunk0, chunk0 + nchunks) of 16 bytes of the old row; nchunks = 0: byte gather
struct KeepPiece { uint32_t chunk0, nchunks; };

// grid = (pieces from piece0 on, groups of four rows -- a wave per row; the row groups beyond the grid are walked in a loop)
template <int W>
__global__ __launch_bounds__(256) void keep_gather_kernel(MatRef M, uint64_t ld, uint32_t p0, uint32_t nrows, const uint32_t *__restrict__ ids,
                                                          const KeepPiece *__restrict__ pieces, uint32_t piece0, uint32_t n,
                                                          uint8_t *__restrict__ stage, uint64_t spitch)
{
    using fp_t = typename std::conditional<W == 1, uint8_t, uint16_t>::type;
    constexpr uint32_t kPer = 16 / W;                              // elements of a lane
    __shared__ uint4 s_span[4][kKeepSpan / 16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t piece = piece0 + blockIdx.x;
    const KeepPiece pc = pieces[piece];
    const uint32_t j0 = piece * (kKeepPiece / W) + lane * kPer;
    uint32_t id[kPer];
#pragma unroll
    for (uint32_t u = 0; u < kPer / 4; ++u) {
        const uint4 v = reinterpret_cast<const uint4 *>(ids + j0)[u];
        id[4 * u] = v.x; id[4 * u + 1] = v.y; id[4 * u + 2] = v.z; id[4 * u + 3] = v.w;
    }
    const uint32_t e0 = pc.chunk0 * kPer;                          // first element of the span
    for (uint32_t rg = blockIdx.y * 4; rg < nrows; rg += gridDim.y * 4) {      // (the same trips for the whole workgroup)
        const uint32_t r = rg + wave;
        const bool ok = r < nrows;
        const uint8_t *row = mat_row(M, p0 + (ok ? r : rg), ld);
        uint32_t out[4] = {0, 0, 0, 0};
        if (pc.nchunks) {
            if (ok)
                for (uint32_t ch = lane; ch < pc.nchunks; ch += 64) s_span[wave][ch] = reinterpret_cast<const uint4 *>(row)[pc.chunk0 + ch];
            __syncthreads();
            const fp_t *s = reinterpret_cast<const fp_t *>(s_span[wave]);
#pragma unroll
            for (uint32_t e = 0; e < kPer; ++e) {
                const uint32_t v = j0 + e < n ? (uint32_t)s[id[e] - e0] : 0u;
                out[e * W / 4] |= v << ((e * 8 * W) & 31u);
            }
            __syncthreads();                                       // (the next trip's loads overwrite the span)
        } else {
            const fp_t *s = reinterpret_cast<const fp_t *>(row);
#pragma unroll
            for (uint32_t e = 0; e < kPer; ++e) {
                const uint32_t v = j0 + e < n ? (uint32_t)s[id[e]] : 0u;
                out[e * W / 4] |= v << ((e * 8 * W) & 31u);
            }
        }
        if (ok)
            *reinterpret_cast<uint4 *>(stage + (uint64_t)r * spitch + (uint64_t)blockIdx.x * kKeepPiece + lane * 16u) =
                make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// chunks [chunk_lo, chunk_lo + nchunks) of 16 bytes of rows [p0, p0 + nrows): the first nstage of them from the stage, zeros
// behind.  grid = (ceil(nchunks / 256), rows; the rows beyond the grid in a loop)
__global__ __launch_bounds__(256) void keep_store_kernel(MatRef M, uint64_t ld, uint32_t p0, uint32_t nrows, const uint8_t *__restrict__ stage,
                                                         uint64_t spitch, uint32_t chunk_lo, uint32_t nstage, uint32_t nchunks)
{
    const uint32_t ch = blockIdx.x * 256u + threadIdx.x;
    if (ch >= nchunks) return;
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ch < nstage) v = *reinterpret_cast<const uint4 *>(stage + (uint64_t)r * spitch + (uint64_t)ch * 16);
        *reinterpret_cast<uint4 *>(mat_row(M, p0 + r, ld) + ((uint64_t)chunk_lo + ch) * 16) = v;
    }
}

// ids: LOCAL genome ids, distinct, all below c->G (the caller checked), n >= 1; the cold rows are raw.  Returns when the rows
// are in place.
int launch_keep(mk_ctx *c, const uint32_t *ids, uint32_t n)
{
    const uint32_t W = c->W, E = kKeepPiece / W;                   // elements per piece
    const uint64_t npieces = ((uint64_t)n + E - 1) / E;
    uint32_t lead = 0;
    while (lead < n && ids[lead] == lead) ++lead;
    const uint64_t piece0 = lead / E;                              // whole pieces of columns that stay where they are
    const uint64_t old_chunks = ((uint64_t)c->G * W + 15) / 16;    // 16-byte chunks of a row that may hold something
    const uint64_t chunk_lo = piece0 * (kKeepPiece / 16), nstage = (npieces - piece0) * (kKeepPiece / 16);
    const uint64_t nchunks = std::max(old_chunks, chunk_lo + nstage) - chunk_lo;          // (chunk_lo + nstage <= ld / 16: ld is whole KiB)
    if (!nchunks) return MK_OK;
    const uint64_t spitch = nstage * 16;
    // the list padded to whole pieces (the padding's elements are written as zeros), and every piece's path
    std::vector<uint32_t> padded(npieces * E, 0u);
    std::copy(ids, ids + n, padded.begin());
    std::vector<KeepPiece> pieces(npieces, KeepPiece{0, 0});
    for (uint64_t q = piece0; q < npieces; ++q) {
        const uint64_t a = q * E, b = std::min<uint64_t>(n, a + E);
        bool asc = true;
        for (uint64_t j = a + 1; j < b && asc; ++j) asc = ids[j] > ids[j - 1];
        if (!asc) continue;
        const uint64_t c0 = (uint64_t)ids[a] * W / 16, c1 = ((uint64_t)ids[b - 1] * W + W + 15) / 16;
        if (c1 - c0 <= kKeepSpan / 16) pieces[q] = KeepPiece{(uint32_t)c0, (uint32_t)(c1 - c0)};
    }
    uint32_t *d_ids = nullptr;
    KeepPiece *d_pieces = nullptr;
    const uint32_t rows_per = nstage ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c->P, (256ull << 20) / spitch)) : c->P;
    int rc = MK_OK;
    if (nstage) {
        // (the staging buffer stays with the context, as for the column transfers)
        MK_TRY(c->d_colstage.grow((uint64_t)rows_per * spitch));
        rc = dev_alloc(&d_ids, padded.size());
        if (rc == MK_OK) rc = dev_alloc(&d_pieces, pieces.size());
        if (rc == MK_OK && hipMemcpyAsync(d_ids, padded.data(), padded.size() * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = MK_ERR_DEVICE;
        if (rc == MK_OK && hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(KeepPiece), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = MK_ERR_DEVICE;
    }
    const MatRef M = mat_ref(c);
    for (uint32_t p0 = 0; p0 < c->P && rc == MK_OK; p0 += rows_per) {
        const uint32_t r = std::min(rows_per, c->P - p0);
        if (nstage) {
            const dim3 grid((uint32_t)(npieces - piece0), std::min<uint32_t>((r + 3) / 4, 65535u));
            if (W == 1) hipLaunchKernelGGL(keep_gather_kernel<1>, grid, dim3(256), 0, c->stream, M, c->ld, p0, r, d_ids, d_pieces, (uint32_t)piece0, n, c->d_colstage, spitch);
            else hipLaunchKernelGGL(keep_gather_kernel<2>, grid, dim3(256), 0, c->stream, M, c->ld, p0, r, d_ids, d_pieces, (uint32_t)piece0, n, c->d_colstage, spitch);
        }
        hipLaunchKernelGGL(keep_store_kernel, dim3((uint32_t)((nchunks + 255) / 256), std::min<uint32_t>(r, 65535u)), dim3(256), 0, c->stream, M, c->ld, p0, r,
                           c->d_colstage, spitch, (uint32_t)chunk_lo, (uint32_t)nstage, (uint32_t)nchunks);
        if (hipGetLastError() != hipSuccess) rc = MK_ERR_DEVICE;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == MK_OK) rc = MK_ERR_DEVICE;
    if (rc == MK_ERR_DEVICE) set_error("genome selection failed: %s", hipGetErrorString(hipGetLastError()));
    dev_free(d_ids); dev_free(d_pieces);
    return rc;
}

}  // namespace mk
