// K6e: representatives of the indexed genomes -- greedy clustering in id order over "one lists the other" (filter_results'
// test, Miekki.cpp:381-384): genome i is a representative unless an earlier representative is linked with it, and then
// rep[i] is the smallest such representative.  Star clusters: every member is linked with its own representative.
//
// Genomes are walked in sets of consecutive ids: a set's rows first, then its ids in order, at most kRepMaxSet at a time
// ("the set" of the three steps below; the rest of the scanned set lies above it), all on one stream:
//   rows:      list_kernel's walk (list_walk.hpp) with a third sink: the wave that walks query q writes the pot bits of every
//              step into row (q's place in the set, not in the chunk) of a bitmap, one bit per genome, the query's own bit
//              cleared.  A wave owns its row and rows are padded to whole steps: plain stores, no bound test, no atomics;
//   below:     one wave per query i of the set: the first set bit of row_i & is_rep over the ids below the set (i lists an
//              earlier, final representative) is folded into rep[i] with min;
//   resolve:   ONE workgroup: the symmetric bit matrix row_i[j] | row_j[i] over the set's own ids and the running
//              representative mask are kept in LDS, and one wave goes through the set's ids in order -- a dependent chain
//              that never leaves the CU;
//   propagate: for every id i that became a representative in this set and every set bit j of row_i above the set,
//              atomicMin(rep + j, i); the new representatives' bits go into is_rep.
//
// The invariant between sets: for an id j not yet walked, rep[j] is the smallest FINAL representative that lists j (or j).
// `below` adds the final representatives that j lists itself, so after it rep[j] != j says "member of an earlier cluster"
// and is final; the rest is decided among the set's own ids.  Every launch reads what EARLIER launches wrote (plain loads);
// the only words several workgroups write in one launch are rep[j] above the set and is_rep, with agent-scope atomics, and
// nothing reads them before the launch is over.  Ids here are local genome numbers; the host adds genome_id_base.
#include "list_walk.hpp"

namespace mk {

namespace {

// (sets made from the index are dense: their chunks carry u32 scores, which the walk takes four genomes per lane)
__global__ __launch_bounds__(256) void rep_rows_kernel(const RepRowsArgs k)
{
    constexpr uint32_t GPL = ListWalk<0>::GPL;
    static_assert(GPL == 4, "two lanes' bits make one byte of a row");
    const ListArgs &a = k.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;
    const uint32_t q = a.q_lo + qi;
    const uint32_t pos = k.chunk_pos + q;                                   // the query's place in the set
    const uint32_t self = k.set_g0 + pos;                                   // ... and the genome it is
    uint8_t *const row = reinterpret_cast<uint8_t *>(k.rows + (uint64_t)pos * k.row_words);
    list_walk<0>(a, q, lane, [&](uint32_t gl, const uint32_t (&)[GPL], uint32_t pot) {
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j)
            if (gl + j == self) pot &= ~(1u << j);                          // a genome lists itself: no link
        const uint32_t up = (uint32_t)__shfl_xor((int)pot, 1);              // lanes 2m, 2m + 1: the two halves of one byte
        if (!(lane & 1u)) row[gl >> 3] = (uint8_t)(pot | (up << 4));        // the wave: 32 contiguous bytes
    });
}

__global__ __launch_bounds__(256) void rep_reset_kernel(uint32_t *__restrict__ rep, uint32_t n, uint32_t *__restrict__ is_rep, uint32_t words)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) rep[i] = i;
    if (i < words) is_rep[i] = 0;
}

// bits [g0, g0 + 32) of a row of `words` words (what lies beyond the row reads as 0)
__device__ __forceinline__ uint32_t row_bits(const uint32_t *__restrict__ row, uint32_t words, uint32_t g0)
{
    const uint32_t w = g0 >> 5, sh = g0 & 31u;
    const uint32_t lo = w < words ? row[w] : 0u;
    if (!sh) return lo;
    const uint32_t hi = w + 1 < words ? row[w + 1] : 0u;
    return (lo >> sh) | (hi << (32u - sh));
}

// one wave per query of the set: the smallest final representative (an id below the set) that the query lists
__global__ __launch_bounds__(256) void rep_below_kernel(const RepArgs k)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= k.n) return;
    const uint32_t *__restrict__ row = k.rows + (uint64_t)i * k.row_words;
    const uint32_t nw = (k.set_g0 + 31u) >> 5;                              // words that hold ids below the set
    for (uint32_t w0 = 0; w0 < nw; w0 += 64) {
        const uint32_t w = w0 + lane;
        uint32_t x = 0;
        if (w < nw) {
            x = row[w] & k.is_rep[w];
            if (w == nw - 1 && (k.set_g0 & 31u)) x &= (1u << (k.set_g0 & 31u)) - 1u;
        }
        const uint64_t hit = __ballot(x != 0);
        if (!hit) continue;                                                 // wave-uniform
        const uint32_t first = (uint32_t)__builtin_ctzll(hit);             // words ascend with the lanes: the first lane has it
        const uint32_t xf = (uint32_t)__shfl((int)x, (int)first);
        if (lane == 0) {
            const uint32_t r = (w0 + first) * 32u + (uint32_t)__builtin_ctz(xf);
            uint32_t *const slot = k.rep + k.set_g0 + i;                    // (this wave's alone in this launch)
            if (r < *slot) *slot = r;
        }
        return;
    }
}

// ONE workgroup.  LDS: m[n][nw] the in-set link matrix (nw = words of n bits), srep[n], todo[nw].
__global__ __launch_bounds__(1024) void rep_resolve_kernel(const RepArgs k)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rep_lds[];
    const uint32_t n = k.n, nw = (n + 31u) >> 5, g0 = k.set_g0;
    uint32_t *const m = rep_lds, *const srep = m + n * nw, *const todo = srep + n;
    const uint32_t tid = threadIdx.x, cells = n * nw;
    const uint32_t words = (k.G + 31u) >> 5;                                // the words of a row that the walk wrote and that hold genomes
    // what every query of the set lists among the set's own ids
    for (uint32_t c = tid; c < cells; c += 1024u) {
        const uint32_t i = c / nw, w = c - i * nw;
        uint32_t x = row_bits(k.rows + (uint64_t)i * k.row_words, words, g0 + 32u * w);
        if (w == nw - 1 && (n & 31u)) x &= (1u << (n & 31u)) - 1u;
        m[c] = x;
    }
    for (uint32_t i = tid; i < n; i += 1024u) srep[i] = k.rep[g0 + i];
    if (tid < nw) todo[tid] = 0;
    __syncthreads();
    // ... or is listed by: every bit to its mirror place too.  In place: a bit met here that another thread has just added is
    // a mirror whose own mirror is the original -- setting it again changes nothing.
    for (uint32_t c = tid; c < cells; c += 1024u) {
        const uint32_t i = c / nw, w = c - i * nw;
        for (uint32_t x = m[c]; x; x &= x - 1u) {
            const uint32_t j = 32u * w + (uint32_t)__builtin_ctz(x);
            atomicOr(m + j * nw + (i >> 5), 1u << (i & 31u));
        }
    }
    __syncthreads();
    // the ids the chain has to visit: not a member of an earlier cluster, and linked with some id of the set
    for (uint32_t c = tid; c < cells; c += 1024u) {
        const uint32_t i = c / nw;
        if (m[c] && srep[i] == g0 + i) atomicOr(todo + (i >> 5), 1u << (i & 31u));
    }
    __syncthreads();
    if (tid < 64) {
        // lane w keeps word w of the set's representatives so far (nw <= 32)
        uint32_t mask = 0;
        const uint32_t td = tid < nw ? todo[tid] : 0u;
        for (uint32_t w = 0; w < nw; ++w) {
            for (uint32_t tw = (uint32_t)__builtin_amdgcn_readlane((int)td, (int)w); tw; tw &= tw - 1u) {
                const uint32_t b = (uint32_t)__builtin_ctz(tw), i = 32u * w + b;
                const uint32_t x = tid < nw ? m[i * nw + tid] & mask : 0u;  // (representatives so far are all below i)
                const uint64_t hit = __ballot(x != 0);
                if (hit) {
                    const uint32_t first = (uint32_t)__builtin_ctzll(hit);
                    const uint32_t xf = (uint32_t)__shfl((int)x, (int)first);
                    if (tid == 0) srep[i] = g0 + first * 32u + (uint32_t)__builtin_ctz(xf);
                } else if (tid == w) {
                    mask |= 1u << b;
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024u) k.rep[g0 + i] = srep[i];
}

// one wave per id of the set: a new representative claims what it lists above the set
__global__ __launch_bounds__(256) void rep_propagate_kernel(const RepArgs k)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (i >= k.n) return;
    const uint32_t id = k.set_g0 + i;
    if (k.rep[id] != id) return;                                            // (the resolve launch is over: a plain load)
    if (lane == 0) atomicOr(k.is_rep + (id >> 5), 1u << (id & 31u));
    const uint32_t *__restrict__ row = k.rows + (uint64_t)i * k.row_words;
    const uint32_t above = k.set_g0 + k.n, words = (k.G + 31u) >> 5;
    for (uint32_t w = (above >> 5) + lane; w < words; w += 64) {
        uint32_t x = row[w];
        if (w == (above >> 5)) x &= ~((1u << (above & 31u)) - 1u);
        for (; x; x &= x - 1u) {
            const uint32_t j = 32u * w + (uint32_t)__builtin_ctz(x);       // (< G: the walk leaves no bit beyond the genomes)
            __hip_atomic_fetch_min(k.rep + j, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

uint32_t rep_row_words(uint32_t G) { return (G + 511u) / 512u * 16u; }
uint64_t rep_resolve_lds(uint32_t n) { const uint64_t nw = (n + 31u) / 32u; return 4ull * (n * nw + n + nw); }

int launch_rep_rows(mk_ctx *c, const RepRowsArgs &k)
{
    const ListArgs &a = k.list;
    if (!a.q_n || !a.G) return MK_OK;
    MK_TRY(walk_range(a));
    if (!k.rows || k.row_words < rep_row_words(a.G)) { set_error("the row pass needs the set's bitmap"); return MK_ERR_ARG; }
    // (there is no kernel for partial counts: a set made from the index never takes the slab schedule)
    if (a.partials || !a.scores) { set_error("bitmap rows are written from a dense chunk's scores only"); return MK_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(rep_rows_kernel, dim3((a.q_n + 3) / 4), dim3(256), 0, c->stream, k);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_rep_reset(mk_ctx *c, uint32_t *d_rep, uint32_t n, uint32_t *d_is_rep)
{
    if (!n) return MK_OK;
    hipLaunchKernelGGL(rep_reset_kernel, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, d_rep, n, d_is_rep, (n + 31u) / 32u);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_rep_resolve(mk_ctx *c, const RepArgs &k)
{
    if (!k.n) return MK_OK;
    if (k.n > kRepMaxSet || (uint64_t)k.set_g0 + k.n > k.G || k.row_words < rep_row_words(k.G)) { set_error("a set of %u ids from %u over %u genomes does not fit the resolve step", k.n, k.set_g0, k.G); return MK_ERR_ARG; }
    const dim3 waves((k.n + 3) / 4), block(256);
    if (k.set_g0) hipLaunchKernelGGL(rep_below_kernel, waves, block, 0, c->stream, k);
    const size_t lds = rep_resolve_lds(k.n);
    MK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rep_resolve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rep_resolve_lds(kRepMaxSet)));
    hipLaunchKernelGGL(rep_resolve_kernel, dim3(1), dim3(1024), lds, c->stream, k);
    hipLaunchKernelGGL(rep_propagate_kernel, waves, block, 0, c->stream, k);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
