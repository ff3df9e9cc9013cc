// K6d: families of genomes -- the connected components of "one lists the other" (single linkage over filter_results' test,
// Miekki.cpp:381-384) -- as a union-find forest in device memory.
//
//   link:    list_kernel's walk (list_walk.hpp: one wave per query over the chunk's scores or partial counts, the f32 screen,
//            the double decision) with another sink: a passing (query, genome) pair is not written anywhere, its two ids are
//            joined in parent[n_ids];
//   levels:  the same walk over up to MK_MAX_LEVELS nested pairs of thresholds at once, a forest per level: a passing pair is
//            joined in the forest of the strictest level it passes (link_levels_kernel);
//   merge:   joins i with other[i] for every i: folds the forest of another shard into this one;
//   labels:  a later launch; label[i] = the root of i = the smallest id of i's family.
//
// The forest.  parent[i] <= i always, a root is its own parent, and the only way a root stops being one is an agent-scope
// compare-and-swap on ITS OWN slot that hooks it under a smaller id -- so a family's root is its smallest id whatever the
// order of the joins, and a slot's successive values are all ancestors of the slot: once an ancestor, always one.  Nothing
// waits for another workgroup: a failed swap returns the parent somebody else gave the root, and the join goes on from there.
// Per-XCD L2s are not coherent and a CU's L1 is never refreshed, so every read of the forest in the link and merge kernels is
// a relaxed agent-scope atomic load and every write an agent-scope atomic.  A stale value would be harmless all the same: it
// is a former parent -- same family, smaller or equal id -- so "same root" read from stale values is still true, and a swap
// that expects a stale root fails and tells the truth.  Path halving replaces a parent by the grandparent just read, an
// ancestor, with such a store (it never touches a root: the slot was seen with a parent other than itself, and stays so).
#include "list_walk.hpp"

namespace mk {

namespace {

__device__ __forceinline__ uint32_t par_load(const uint32_t *p, uint32_t i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void par_store(uint32_t *p, uint32_t i, uint32_t v) { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see (a former root at worst), halving the path on the way
__device__ __forceinline__ uint32_t find_root(uint32_t *p, uint32_t x)
{
    for (;;) {
        const uint32_t px = par_load(p, x);
        if (px == x) return x;
        const uint32_t gp = par_load(p, px);
        if (gp == px) return px;
        par_store(p, x, gp);                                                // gp < px < x: an ancestor of x
        x = gp;
    }
}

// join the families of x and y: the larger root goes under the smaller
__device__ __forceinline__ void unite(uint32_t *p, uint32_t x, uint32_t y)
{
    for (;;) {
        x = find_root(p, x);
        y = find_root(p, y);
        if (x == y) return;
        if (x < y) { const uint32_t t = x; x = y; y = t; }                   // x: the larger
        uint32_t seen = x;
        if (__hip_atomic_compare_exchange_strong(p + x, &seen, y, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        x = seen;                                                           // x had a parent already: go on from it
    }
}

// Per step of the walk: the root of the query's id is read ONCE, the roots of the passing genomes once each, and the wave
// agrees on the smallest of them; only roots other than that one are hooked under it, each with a swap on its own slot.  Lanes
// whose genomes already share the query's root issue no atomic -- a clique of n copies is n - 1 successful swaps in all, not
// n^2 on one word.  All 64 lanes call it (the shuffles), with bit j of pot = genome id0 + j is joined with idq.
template <uint32_t GPL>
__device__ __forceinline__ void link_step(uint32_t *p, uint32_t idq, uint32_t id0, uint32_t pot, uint32_t lane)
{
    const uint32_t rq = find_root(p, idq);                                  // (every lane the same address: one access)
    uint32_t r[GPL], low = rq;
#pragma unroll
    for (uint32_t j = 0; j < GPL; ++j) {
        r[j] = rq;
        if ((pot >> j) & 1u) { r[j] = find_root(p, id0 + j); low = min(low, r[j]); }
    }
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) low = min(low, (uint32_t)__shfl_xor(low, o));
#pragma unroll
    for (uint32_t j = 0; j < GPL; ++j)
        if (r[j] != low && (j == 0 || r[j] != r[j - 1])) unite(p, r[j], low);
    if (lane == 0 && rq != low) unite(p, rq, low);
}

// a genome lists itself: nothing to join
template <uint32_t GPL>
__device__ __forceinline__ uint32_t without_self(uint32_t pot, uint32_t id0, uint32_t idq)
{
#pragma unroll
    for (uint32_t j = 0; j < GPL; ++j)
        if (id0 + j == idq) pot &= ~(1u << j);
    return pot;
}

template <int SRC>
__global__ __launch_bounds__(256) void link_kernel(const LinkArgs k)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    const ListArgs &a = k.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;
    const uint32_t q = a.q_lo + qi;
    const uint32_t idq = k.query_ids[q];
    uint32_t *const p = k.parent;
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&)[GPL], uint32_t pot) {
        pot = without_self<GPL>(pot, gl + a.genome_id_base, idq);
        if (__ballot(pot != 0) == 0) return;                                // wave-uniform
        link_step<GPL>(p, idq, gl + a.genome_id_base, pot, lane);
    });
}

// Nested levels from one walk.  The walk runs at level 0's thresholds, the loosest, so pot is "passes level 0"; the levels'
// thresholds only rise, so the levels a pair passes are 0 .. d, and the pair is joined ONCE, in forest d (folding the forests
// strict to loose afterwards, launch_link_merge, gives every looser level the pair as well).  d is found with the reference's
// two double operations (list_walk.hpp:77-78) and kept as one nibble per genome -- GPL <= 8: one word -- and the roots live
// inside the level loop only, so nothing is held per level.  The loop over the levels is wave-uniform: a level none of the
// wave's genomes stops at is skipped by a ballot, and in a level that is entered all 64 lanes make link_step's shuffles.
template <int SRC>
__global__ __launch_bounds__(256) void link_levels_kernel(const LinkLevelsArgs k)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    static_assert(GPL <= 8 && MK_MAX_LEVELS <= 16, "a depth nibble per genome in one word");
    const ListArgs &a = k.link.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;
    const uint32_t q = a.q_lo + qi;
    const uint32_t idq = k.link.query_ids[q];
    const uint32_t n_levels = k.n_levels;
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
        const uint32_t id0 = gl + a.genome_id_base;
        pot = without_self<GPL>(pot, id0, idq);
        if (__ballot(pot != 0) == 0) return;                                // wave-uniform
        uint32_t depth = 0;                                                 // nibble j: the strictest level genome gl + j passes
        if (pot != 0 && n_levels > 1) {
            double inter[GPL];
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j) {
                inter[j] = 0.0;
                if ((pot >> j) & 1u) {                                      // (a set bit: gl + j < G)
                    const double jac = (double)s[j] / (double)a.sketch_size[gl + j];        // Miekki.cpp:382-383
                    inter[j] = jac * (double)a.genome_size[gl + j];
                }
            }
            uint32_t still = pot;                                           // passes every level so far
            for (uint32_t l = 1; l < n_levels; ++l) {
                const uint32_t ms = k.levels[l].min_score;
                const double mi = k.levels[l].min_intersection;
#pragma unroll
                for (uint32_t j = 0; j < GPL; ++j) {
                    if (!(s[j] >= ms && !(inter[j] < mi))) still &= ~(1u << j);             // Miekki.cpp:381, 384
                    depth += ((still >> j) & 1u) << (4 * j);
                }
            }
        }
        for (uint32_t l = 0; l < n_levels; ++l) {
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j) mine |= (uint32_t)(((depth >> (4 * j)) & 15u) == l) << j;
            mine &= pot;
            if (__ballot(mine != 0) == 0) continue;                         // wave-uniform
            link_step<GPL>(k.link.parent + (size_t)l * k.n_ids, idq, id0, mine, lane);
        }
    });
}

__global__ __launch_bounds__(256) void link_reset_kernel(uint32_t *__restrict__ parent, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) parent[i] = i;
}

__global__ __launch_bounds__(256) void link_merge_kernel(uint32_t *parent, const uint32_t *__restrict__ other, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = other[i];
    if (o < n && o != i) unite(parent, i, o);                               // (a forest's parent[i] <= i; anything else is not followed)
}

// the forest is at rest (the launches that wrote it are over): plain loads
__global__ __launch_bounds__(256) void link_labels_kernel(const uint32_t *__restrict__ parent, uint32_t n, uint32_t *__restrict__ label)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t x = i;
    for (uint32_t px = parent[x]; px < x; px = parent[x]) x = px;           // (px < x: a walk ends even over a forest that is none)
    label[i] = x;
}

inline dim3 blocks_of(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

int launch_link(mk_ctx *c, const LinkArgs &k)
{
    const char *missing = k.parent && k.query_ids ? nullptr : "the link pass needs the forest and the queries' ids";
    return launch_walk(c, k.list, "links", missing, [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(link_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

int launch_link_levels(mk_ctx *c, const LinkLevelsArgs &k)
{
    const char *missing = !k.link.parent || !k.link.query_ids ? "the link pass needs the forests and the queries' ids"
                          : k.n_levels < 1 || k.n_levels > MK_MAX_LEVELS ? "the link pass takes 1 .. 8 levels" : nullptr;
    return launch_walk(c, k.link.list, "links", missing, [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(link_levels_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

int launch_link_reset(mk_ctx *c, uint32_t *d_parent, uint32_t n)
{
    if (!n) return MK_OK;
    hipLaunchKernelGGL(link_reset_kernel, blocks_of(n), dim3(256), 0, c->stream, d_parent, n);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_link_merge(mk_ctx *c, uint32_t *d_parent, const uint32_t *d_other, uint32_t n)
{
    if (!n) return MK_OK;
    hipLaunchKernelGGL(link_merge_kernel, blocks_of(n), dim3(256), 0, c->stream, d_parent, d_other, n);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_link_labels(mk_ctx *c, const uint32_t *d_parent, uint32_t n, uint32_t *d_label)
{
    if (!n) return MK_OK;
    hipLaunchKernelGGL(link_labels_kernel, blocks_of(n), dim3(256), 0, c->stream, d_parent, n, d_label);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
