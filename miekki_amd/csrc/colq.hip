// Query sets made from stored columns (mk_qset_from_index / mk_qset_from_columns): the column of an indexed genome IS the
// gated sketch query_sequence would compute for the genome's sequence -- insert_sequences and query_sequence share
// minhash_sketch_partition (Miekki.cpp:281, 320), the stored byte of partition p is the query's first[p] (228-239, 291), and
// the Bloom gate (135-146) passes every active partition of a genome that was inserted (295-299, 121-131; no cell ever
// returns to zero).  So the "sketch" step of such a set is a gather: matrix columns -> the dense query layout
// scan_dense_lut_kernel consumes, dense[group][p][4] (native fp_t, pad slots = empty), and the count of non-empty
// partitions per query, through per-workgroup partial sums as dense_batch_kernel counts them (sketch.hip).
#include <algorithm>
#include <type_traits>

#include "mk_internal.hpp"

namespace mk {

// rows of the matrix one workgroup turns into 1 KiB of every group's vector
template <int W> struct ColRows { static constexpr uint32_t value = 1024u / (4u * W); };

// 4 slots of fingerprints (native fp_t, `words` = one dword for W = 1, two for W = 2) with the slots from `nvalid` on made
// empty; returns through ne[] which slots are not empty
template <int W>
__device__ __forceinline__ void mask_slots(uint32_t (&words)[W], uint32_t nvalid, uint32_t empty, bool (&ne)[4])
{
    constexpr uint32_t bits = 8 * W, fmask = (1u << bits) - 1u;
#pragma unroll
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t wi = s * W / 4, sh = (s * bits) & 31u;
        uint32_t v = (words[wi] >> sh) & fmask;
        if (s >= nvalid) { v = empty; words[wi] = (words[wi] & ~(fmask << sh)) | (empty << sh); }
        ne[s] = v != empty;
    }
}

// A run of m <= 64 CONSECUTIVE genomes g0 .. g0 + m - 1 into the sixteen groups that start at `dense` (slot 0 of the first
// group = genome g0).  A row's piece is m W contiguous bytes: the workgroup reads its rows' pieces as the aligned 16-byte
// chunks that cover them (up to eight loads in flight per lane), lays them out in LDS (skewed: see row_at), and every lane then takes the 4 W
// bytes of one (group, row) out of LDS at the piece's byte shift -- two or three dwords and v_alignbyte -- four (two) rows
// at a time, so that a wave stores 1 KiB of one group's vector with 16-byte stores.  grid = ceil(P / ColRows<W>).
// VEC: a group's vector is a multiple of 16 bytes (P >= 4 / W; P is a power of two, so a lane's rows are then all inside the
// matrix or all outside); otherwise -- two partitions of one-byte fingerprints -- a dword per (group, row).
template <int W, bool VEC>
__global__ __launch_bounds__(256) void column_gather_kernel(MatRef M, uint64_t ld, uint32_t P, uint32_t g0, uint32_t m, uint32_t empty,
                                                            uint8_t *__restrict__ dense, uint32_t *__restrict__ partial, uint32_t nblk)
{
    constexpr uint32_t kRows = ColRows<W>::value, kC = 4 * W + 1, kPer = 16 / (4 * W);   // chunks per row at most, rows per 16-byte store
    // A row takes kPitch dwords of LDS, and every kPer rows one dword more (row_at): in the read-out lane L takes rows
    // L kPer .. L kPer + kPer - 1, so neighbouring lanes are kPer kPitch + 1 dwords apart -- 81 (W = 1), 73 (W = 2), odd:
    // the 32 lanes that share an LDS cycle fall on 32 different banks.
    constexpr uint32_t kPitch = kC * 4;
    auto row_at = [](uint32_t row) { return row * kPitch + row / kPer; };
    __shared__ uint32_t s_in[kRows * kPitch + kRows / kPer];
    const uint32_t tid = threadIdx.x, p0 = blockIdx.x * kRows;
    const uint32_t nrows = min(kRows, P - p0);
    const uint64_t byte0 = (uint64_t)g0 * W, a0 = byte0 & ~15ull;
    const uint32_t shift = (uint32_t)(byte0 - a0);
    const uint32_t C = (uint32_t)(((uint64_t)(g0 + m) * W - a0 + 15) / 16);               // <= kC; a0 + 16 C <= ld (ld is a multiple of 1 KiB)
    const uint32_t items = nrows * C;                                                      // <= 2048
    uint4 v[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t i = min(tid + 256 * u, items - 1);          // (every lane loads, so that the eight loads go out together)
        const uint32_t row = i / C, ch = i - row * C;
        v[u] = *reinterpret_cast<const uint4 *>(mat_row(M, p0 + row, ld) + a0 + (uint64_t)ch * 16);
    }
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t i = tid + 256 * u;
        if (i < items) {
            const uint32_t row = i / C, ch = i - row * C;
            uint32_t *d = s_in + row_at(row) + ch * 4;
            d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
        }
    }
    __syncthreads();
    const uint32_t lane = tid & 63u, r0 = lane * kPer;
#pragma unroll
    for (uint32_t it = 0; it < 4; ++it) {
        const uint32_t gr = 4 * it + (tid >> 6);                   // one group per wave and round
        if (gr * 4 >= m) break;                                    // (wave-uniform)
        const uint32_t nvalid = min(4u, m - gr * 4);
        uint32_t out[4];
        uint32_t cnt[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
            const uint32_t row = r0 + k;
            const bool ok = row < nrows;
            const uint32_t o = shift + gr * 4 * W;                 // byte of the piece in its row
            uint32_t words[W];
            if (ok) {
                const uint32_t *d = s_in + row_at(row) + (o >> 2);
                uint32_t lo = d[0];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint32_t hi = d[w + 1];
                    words[w] = __builtin_amdgcn_alignbyte(hi, lo, o & 3u);
                    lo = hi;
                }
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) words[w] = W == 1 ? empty * 0x01010101u : empty * 0x00010001u;
            }
            bool ne[4];
            mask_slots<W>(words, nvalid, empty, ne);
#pragma unroll
            for (uint32_t s = 0; s < 4; ++s) cnt[s] += (uint32_t)__popcll(__ballot(ok && ne[s]));
#pragma unroll
            for (int w = 0; w < W; ++w) out[k * W + w] = words[w];
        }
        uint8_t *dst = dense + ((uint64_t)gr * P + p0 + r0) * 4 * W;
        if constexpr (VEC) {
            if (r0 < nrows) *reinterpret_cast<uint4 *>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kPer; ++k)
                if (r0 + k < nrows) {
#pragma unroll
                    for (int w = 0; w < W; ++w) reinterpret_cast<uint32_t *>(dst)[k * W + w] = out[k * W + w];
                }
        }
        if (lane < nvalid) {
            const uint32_t c = lane == 0 ? cnt[0] : lane == 1 ? cnt[1] : lane == 2 ? cnt[2] : cnt[3];
            partial[(uint64_t)(gr * 4 + lane) * nblk + blockIdx.x] = c;
        }
    }
}

// The general path, for any m <= 64 slots: a lane owns one group (tid & 15) and walks every sixteenth row of the
// workgroup's rows, fetching its four slots' fingerprints one by one through `fetch(p, slot)`; 4 W bytes stored per
// (group, row).  Same grid, same partial sums.
template <int W, typename Fetch>
__device__ __forceinline__ void fill_slots(uint32_t P, uint32_t m, uint32_t empty, uint8_t *__restrict__ dense, uint32_t *__restrict__ partial,
                                           uint32_t nblk, Fetch fetch)
{
    constexpr uint32_t kRows = ColRows<W>::value;
    __shared__ uint32_t s_cnt[64];
    const uint32_t tid = threadIdx.x, gr = tid & 15u, p0 = blockIdx.x * kRows;
    const uint32_t nrows = min(kRows, P - p0);
    if (tid < 64) s_cnt[tid] = 0;
    __syncthreads();
    if (gr * 4 < m) {
        const uint32_t nvalid = min(4u, m - gr * 4);
        uint32_t cnt[4] = {0, 0, 0, 0};
        for (uint32_t row = tid >> 4; row < nrows; row += 16) {
            const uint32_t p = p0 + row;
            uint32_t words[W];
#pragma unroll
            for (int w = 0; w < W; ++w) words[w] = 0;
#pragma unroll
            for (uint32_t s = 0; s < 4; ++s) {
                const uint32_t f = s < nvalid ? fetch(p, gr * 4 + s) : empty;
                words[s * W / 4] |= f << ((s * 8 * W) & 31u);
                cnt[s] += f != empty ? 1u : 0u;
            }
            uint32_t *dst = reinterpret_cast<uint32_t *>(dense + ((uint64_t)gr * P + p) * 4 * W);
#pragma unroll
            for (int w = 0; w < W; ++w) dst[w] = words[w];
        }
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) atomicAdd(&s_cnt[gr * 4 + s], cnt[s]);
    }
    __syncthreads();
    if (tid < m) partial[(uint64_t)tid * nblk + blockIdx.x] = s_cnt[tid];
}

// byte gather: the slots' genomes ids[0 .. m) in any order, repeats included
template <int W>
__global__ __launch_bounds__(256) void column_gather_any_kernel(MatRef M, uint64_t ld, uint32_t P, const uint32_t *__restrict__ ids, uint32_t m,
                                                                uint32_t empty, uint8_t *__restrict__ dense, uint32_t *__restrict__ partial,
                                                                uint32_t nblk)
{
    using fp_t = typename std::conditional<W == 1, uint8_t, uint16_t>::type;
    fill_slots<W>(P, m, empty, dense, partial, nblk, [&](uint32_t p, uint32_t slot) {
        return (uint32_t) reinterpret_cast<const fp_t *>(mat_row(M, p, ld))[ids[slot]];
    });
}

// from a caller's block cols[p][n] in dump_disk's byte order (16-bit values big-endian; what mk_index_export_genomes
// produces): slots q0 .. q0 + m of it
template <int W>
__global__ __launch_bounds__(256) void dense_from_columns_kernel(const uint8_t *__restrict__ cols, uint32_t n, uint32_t q0, uint32_t P, uint32_t m,
                                                                 uint32_t empty, uint8_t *__restrict__ dense, uint32_t *__restrict__ partial,
                                                                 uint32_t nblk)
{
    fill_slots<W>(P, m, empty, dense, partial, nblk, [&](uint32_t p, uint32_t slot) {
        const uint8_t *s = cols + ((uint64_t)p * n + q0 + slot) * W;
        return W == 1 ? (uint32_t)s[0] : ((uint32_t)s[0] << 8 | s[1]);
    });
}

// nent[q] = sum of the query's partial sums; grid = queries
__global__ __launch_bounds__(256) void column_count_kernel(const uint32_t *__restrict__ partial, uint32_t nblk, uint32_t *__restrict__ nent)
{
    __shared__ uint32_t s_sum[4];
    uint32_t v = 0;
    for (uint32_t i = threadIdx.x; i < nblk; i += 256) v += partial[(uint64_t)blockIdx.x * nblk + i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63u) == 0) s_sum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) nent[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

uint32_t column_blocks(const mk_ctx *c) { return (c->P + 1024u / (4u * c->W) - 1) / (1024u / (4u * c->W)); }

// The gather of a whole set: slots [q, q + 64) at a time.  A block of slots whose genomes are consecutive (what the
// all-vs-all drivers hand over) takes the run kernel, any other the byte gather.  h_ids / d_ids: the slots' LOCAL genome
// ids, all below c->G (the caller checked); d_partial: nq x column_blocks(c) words.
int launch_column_gather(mk_ctx *c, const uint32_t *h_ids, const uint32_t *d_ids, uint32_t nq, uint8_t *d_dense, uint32_t *d_partial,
                         uint32_t *d_nent)
{
    if (!nq) return MK_OK;
    const uint32_t nblk = column_blocks(c);
    const uint64_t group_bytes = (uint64_t)c->P * 4 * c->W;
    const bool vec = group_bytes % 16 == 0;
    const MatRef M = mat_ref(c);
    for (uint32_t q = 0; q < nq; q += 64) {
        const uint32_t m = std::min(64u, nq - q);
        bool run = (uint64_t)h_ids[q] + m <= c->G;
        for (uint32_t j = 1; j < m && run; ++j) run = h_ids[q + j] == h_ids[q] + j;
        uint8_t *dense = d_dense + (uint64_t)(q / 4) * group_bytes;
        uint32_t *partial = d_partial + (uint64_t)q * nblk;
        if (run) {
#define MK_COLQ(W_, V_) hipLaunchKernelGGL((column_gather_kernel<W_, V_>), dim3(nblk), dim3(256), 0, c->stream, M, c->ld, c->P, h_ids[q], m, c->empty, dense, partial, nblk)
            if (c->W == 2) MK_COLQ(2, true);
            else if (vec) MK_COLQ(1, true);
            else MK_COLQ(1, false);
#undef MK_COLQ
        } else {
            if (c->W == 1) hipLaunchKernelGGL(column_gather_any_kernel<1>, dim3(nblk), dim3(256), 0, c->stream, M, c->ld, c->P, d_ids + q, m, c->empty, dense, partial, nblk);
            else hipLaunchKernelGGL(column_gather_any_kernel<2>, dim3(nblk), dim3(256), 0, c->stream, M, c->ld, c->P, d_ids + q, m, c->empty, dense, partial, nblk);
        }
    }
    hipLaunchKernelGGL(column_count_kernel, dim3(nq), dim3(256), 0, c->stream, d_partial, nblk, d_nent);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_dense_from_columns(mk_ctx *c, const uint8_t *d_cols, uint32_t nq, uint8_t *d_dense, uint32_t *d_partial, uint32_t *d_nent)
{
    if (!nq) return MK_OK;
    const uint32_t nblk = column_blocks(c);
    const uint64_t group_bytes = (uint64_t)c->P * 4 * c->W;
    for (uint32_t q = 0; q < nq; q += 64) {
        const uint32_t m = std::min(64u, nq - q);
        uint8_t *dense = d_dense + (uint64_t)(q / 4) * group_bytes;
        uint32_t *partial = d_partial + (uint64_t)q * nblk;
        if (c->W == 1) hipLaunchKernelGGL(dense_from_columns_kernel<1>, dim3(nblk), dim3(256), 0, c->stream, d_cols, nq, q, c->P, m, c->empty, dense, partial, nblk);
        else hipLaunchKernelGGL(dense_from_columns_kernel<2>, dim3(nblk), dim3(256), 0, c->stream, d_cols, nq, q, c->P, m, c->empty, dense, partial, nblk);
    }
    hipLaunchKernelGGL(column_count_kernel, dim3(nq), dim3(256), 0, c->stream, d_partial, nblk, d_nent);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
