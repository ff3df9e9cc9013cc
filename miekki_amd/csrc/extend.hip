// mk_index_extend: the columns of one index behind the columns of another.  The matrix is partition-major and a row holds W
// bytes per genome, so in every one of the 2^h rows the nbytes = G_src * W bytes at the front of src's row go to byte offset
// off = G_dst * W of dst's row -- two pitches, rows on either side in HBM or in host memory (mat_row), both matrices in the
// device's own byte order: a byte move.  off has any alignment; the rows themselves start on 16-byte boundaries.
//
// extend_place_kernel cuts dst's row into its 16-byte WORDS from the one that holds byte `off` on; a wave takes a PIECE of 64
// of them (1 KiB), a lane one word, a workgroup the same piece of four rows, the row groups beyond the grid in a loop (the
// shape of keep_store_kernel).  A word that lies inside [off, off + nbytes) is one 16-byte store.  Where its bytes come from:
// src's byte (word - off), which sits sh = (16 - off % 16) % 16 bytes into one of src's words for EVERY word of the row --
// so a lane makes TWO ALIGNED 16-byte loads of src (one when sh = 0) and shifts the 32 bytes right by sh, rather than one
// unaligned load: aligned loads are what the compiler can be told to emit, the second load of a lane is the first of its
// neighbour (it comes from L1 / L2, not from memory again), and the shift is a handful of ALU operations under a move that
// waits for memory.  The second load ends at most at src's byte roundup(nbytes, 16), inside the row's pitch (whole KiB).
// The words at the two ends that [off, off + nbytes) covers in part -- up to 15 bytes in front of the first whole word, up to
// 15 behind the last, or the whole span when it holds no whole word -- are stored byte by byte by the lanes that own them.
// Nothing outside [off, off + nbytes) of a row is stored: the columns in front are dst's genomes, those behind stay zero.
#include <algorithm>

#include "mk_internal.hpp"

namespace mk {

constexpr uint32_t kExtendPiece = 1024;  // bytes of a destination row one wave stores: 64 lanes x 16 B

// grid = (pieces of the span, groups of four rows -- a wave per row; the row groups beyond the grid are walked in a loop)
__global__ __launch_bounds__(256) void extend_place_kernel(MatRef D, uint64_t ld_dst, MatRef S, uint64_t ld_src, uint32_t nrows, uint64_t off,
                                                           uint64_t nbytes)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t end = off + nbytes;
    const uint64_t w = (off & ~15ull) + (uint64_t)blockIdx.x * kExtendPiece + lane * 16u;      // this lane's word of the row
    if (w >= end) return;
    const uint32_t sh = (uint32_t)((16u - (off & 15u)) & 15u);    // src's byte (w - off) lies sh bytes into a word of src
    const bool whole = w >= off && w + 16 <= end;
    const uint32_t ds = sh >> 2, bs = (sh & 3u) * 8u;
    for (uint32_t r = blockIdx.y * 4 + wave; r < nrows; r += gridDim.y * 4) {
        uint8_t *drow = mat_row(D, r, ld_dst);
        const uint8_t *srow = mat_row(S, r, ld_src);
        if (whole) {
            const uint64_t s = w - off - sh;                       // (w - off = sh + a multiple of 16)
            const uint4 a = *reinterpret_cast<const uint4 *>(srow + s);
            uint4 o = a;
            if (sh) {
                const uint4 b = *reinterpret_cast<const uint4 *>(srow + s + 16);
                const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                uint32_t t[5];
#pragma unroll
                for (uint32_t i = 0; i < 5; ++i) t[i] = ds == 0 ? v[i] : ds == 1 ? v[i + 1] : ds == 2 ? v[i + 2] : v[i + 3];
                o = make_uint4(__funnelshift_r(t[0], t[1], bs), __funnelshift_r(t[1], t[2], bs), __funnelshift_r(t[2], t[3], bs),
                               __funnelshift_r(t[3], t[4], bs));
            }
            *reinterpret_cast<uint4 *>(drow + w) = o;
        } else {
            const uint64_t b0 = w > off ? w : off, b1 = w + 16 < end ? w + 16 : end;
            for (uint64_t b = b0; b < b1; ++b) drow[b] = srow[b - off];
        }
    }
}

// src's columns [0, src->G) behind dst's columns [0, dst->G): dst has the capacity, both have raw cold rows, src's stream is
// idle (the caller saw to all three); queued on dst's stream
int launch_extend_place(mk_ctx *dst, const mk_ctx *src)
{
    const uint64_t off = (uint64_t)dst->G * dst->W, nbytes = (uint64_t)src->G * src->W;
    if (!nbytes) return MK_OK;
    if (off + nbytes > dst->ld || nbytes > src->ld) { set_error("index join: the rows do not hold the columns"); return MK_ERR_STATE; }
    const uint64_t pieces = (off + nbytes - (off & ~15ull) + kExtendPiece - 1) / kExtendPiece;
    const dim3 grid((uint32_t)pieces, std::min<uint32_t>((dst->P + 3) / 4, 65535u));
    hipLaunchKernelGGL(extend_place_kernel, grid, dim3(256), 0, dst->stream, mat_ref(dst), dst->ld, mat_ref(src), src->ld, dst->P, off, nbytes);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
