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
//   mark:    table_pass.hpp's walks, the mark a saturating byte increment.  There is no byte atomic: a compare-and-swap loop
//            on the containing dword, agent scope, relaxed, adds 1 to the one byte, leaves the other three as they are read, and
//            stops when the byte reads 255.  (Not an add with an undo after overflow: between the two a wrapped byte reads 0 to a
//            third lane, which would add to it.)  FILTER: the loop's first expected value comes from a plain load; a byte that
//            reads 255 there cannot be stale -- counters never fall inside a pass -- and no atomic is issued; a stale smaller
//            value costs one failed compare-and-swap, which returns the fresh dword, never a wrong count.  Without the filter
//            the first expected value is 0 and the first compare-and-swap fetches the dword.
//   profile: table_pass.hpp's pass with a byte for a cell.  One byte: staged, the 256-byte slices of 32 rows at a time, and a
//            lane reads one LDS byte per fingerprint.  Two bytes: a row's slice is 64 KiB and the bytes are looked up where they
//            lie.
//            Pass 0: per lane covered += m > 0 and sum += m (a chunk has at most 2^24 rows: 255 * rows fits 32 bits), then one
//            relaxed agent-scope add per genome and chunk for each (sum: 64 bits).
//            Passes 1..8: the median by bisection on t, no histogram.  lo = 1, hi = 255 per genome in device memory; a step
//            takes mid = (lo + hi + 1) / 2, a pass counts m >= mid[g] (a lane reads its genomes' mid once), and a small kernel
//            sets lo = mid where the count is at least covered / 2 + 1, else hi = mid - 1.  After 8 steps median = covered ? lo
//            : 0.  All 8 steps run whatever the data; nothing waits on the host in between.
//   cells:   a reduction over the table: its non-zero bytes and its bytes of 255.
#include <algorithm>
#include <cstdlib>

#include "table_pass.hpp"

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

// the table of bytes as the pass reads it (table_pass.hpp)
struct ByteTable {
    using Cell = uint8_t;
    static constexpr uint32_t kCellBits = 8;
    static __device__ __forceinline__ void clear_empty(uint4 &last) { last.w &= 0x00ffffffu; }   // the slice's last byte is `empty`'s
    static __device__ __forceinline__ uint32_t lookup(const uint8_t *sl, uint32_t v) { return sl[v]; }
};

// BISECT false: pass 0, count[g] += #{ m > 0 }, sum[g] += m.  BISECT true: count[g] += #{ m >= mid[g] } (mid >= 1).  A lane's
// second word per genome is the sum of its bytes, or the threshold read once from mid.
template <bool BISECT>
struct DepthCount {
    const uint32_t *mid;
    uint32_t *count;
    unsigned long long *sum;
    __device__ __forceinline__ uint32_t start(uint32_t g, uint32_t G) const { return BISECT ? (g < G ? mid[g] : 1u) : 0u; }
    static __device__ __forceinline__ void add(uint32_t &cnt, uint32_t &aux, uint32_t m)
    {
        cnt += m >= (BISECT ? aux : 1u);
        if (!BISECT) aux += m;
    }
    __device__ __forceinline__ void flush(uint32_t cnt, uint32_t aux, uint32_t g0, uint32_t j) const
    {
        (void)__hip_atomic_fetch_add(count + g0 + j, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!BISECT) (void)__hip_atomic_fetch_add(sum + g0 + j, (unsigned long long)aux, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

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
    return launch_table_mark<uint8_t, bump<false>, bump<true>>(c, qs, depth_filter(), d_mult);
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
    PassGrid grid;
    MK_TRY(table_pass_grid<ByteTable>(c, "MIEKKI_DEPTH_ROWS", &grid, 1u << 24));      // (2^24 rows at the most: a lane's sum of bytes fits 32 bits)
    const uint32_t steps = depth_steps();
    // [sum: G x 8 bytes][covered: G][count: G][lo: G][hi: G][mid: G]
    unsigned long long *d_sum = reinterpret_cast<unsigned long long *>(d_scratch);
    uint32_t *d_cov = d_scratch + (size_t)G * 2, *d_cnt = d_cov + G, *d_lo = d_cnt + G, *d_hi = d_lo + G, *d_mid = d_hi + G;
    MK_HIP(hipMemsetAsync(d_scratch, 0, (size_t)G * 16, c->stream));       // sum, covered, count
    const dim3 block(256), sgrid((G + 255) / 256);
    launch_table_pass<ByteTable>(c, grid, d_mult, DepthCount<false>{nullptr, d_cov, d_sum});
    for (uint32_t step = 0;; ++step) {
        hipLaunchKernelGGL(depth_step_kernel, sgrid, block, 0, c->stream, G, step, steps, d_cov, d_sum, d_cnt, d_lo, d_hi, d_mid, d_out);
        if (step == steps) break;
        launch_table_pass<ByteTable>(c, grid, d_mult, DepthCount<true>{d_mid, d_cnt, nullptr});
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
