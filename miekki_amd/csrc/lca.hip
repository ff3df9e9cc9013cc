// K6h: reads placed in a taxonomy by LOWEST COMMON ANCESTOR -- per node, how many queries have it as the deepest node that
// holds all their hits, the matches of their best hits, and their hits -- as three 64-bit counters per node in device memory,
// and, where asked for, the node of every query.
//
//   lca:  tally.hip's walk with three arrays more: leaf[g] = the deepest node that holds local genome g or MK_NO_NODE (left
//         out: the genome is not there for this pass), parent[v], hi[v].  A passing pair is not written anywhere.  The best
//         hit, the load of a lane's leaves and the add to a counter are walk_best.hpp's, shared with tally.hip and clade.hip.
//
// No tree search.  The nodes are nested intervals of ids, so the deepest node that holds a set of genomes is the deepest one
// that holds its smallest id a and its largest id b: the walk keeps one minimum and one maximum per lane, the wave reduces
// them, and lane 0 climbs `parent` from leaf[a] until hi > b (every node on the way holds a, so lo <= a <= b needs no look).
// The climb takes at most depth + 1 steps, the depth the host found when it derived `parent`.  A climb that leaves the forest
// puts the read in the last slot, "above every node".  No LDS, no scratch, no memory per read, no capacity.
//
// best'(q) is clade.hip's: a left-out genome never becomes a lane's best.  THE MARGIN m < 100 keeps of the passing genomes
// those whose intersection is within m percent of the best one's, x*: inter * 100.0 >= x* * (double)(100 - m), two products and
// no sum, so nothing for the compiler to contract.  x* is known only after the walk: a SECOND walk over the same scores
// recomputes every passing genome's intersection through the one function the first walk used (WalkBest::intersection) and
// keeps minimum, maximum and count of the kept ones.  It is taken wave-uniformly, and only when m < 100 and the query lists
// more than one genome: with m = 100 or one hit the first walk's minimum, maximum and count are the answer.
//
// The counters are added to by walk_best.hpp's count() (64-bit, agent scope, relaxed, no return): three adds per assigned
// query, from lane 0.
#include "walk_best.hpp"

namespace mk {

namespace {

// minimum, maximum and sum over the 64 lanes; a lane that holds nothing brings 0xffffffff, 0, 0
__device__ __forceinline__ void wave_span(uint32_t &lo, uint32_t &hi, uint32_t &cnt)
{
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor(lo, o));
        hi = max(hi, (uint32_t)__shfl_xor(hi, o));
        cnt += (uint32_t)__shfl_xor(cnt, o);
    }
}

template <int SRC>
__global__ __launch_bounds__(256) void lca_kernel(const LcaArgs k)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    const ListArgs &a = k.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;                                               // (wave-uniform: every lane of a wave reaches every shuffle)
    const uint32_t q = a.q_lo + qi;
    // ---- walk 1: the best of this lane's listed genomes that have a leaf; count, smallest and largest id of all of them
    WalkBest best;
    uint32_t lo = 0xffffffffu, hi = 0, cnt = 0;
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
        uint32_t lf[GPL];
        if (!pot || !lane_map_row<GPL>(k.leaf, k.map_n, gl, lf)) return;   // (no shuffle in this sink: lanes may leave alone)
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) {
            if (!((pot >> j) & 1u) || lf[j] == MK_NO_NODE) continue;       // (a set bit: gl + j < G)
            const uint32_t g = gl + j;
            best.meet(a, g, s[j]);
            lo = min(lo, g);
            hi = g;                                                        // (ids ascend along the walk)
            ++cnt;
        }
    });
    uint32_t none = 0;
    best.wave_merge(none);
    wave_span(lo, hi, cnt);                                                // (now wave-uniform: L'(q)'s span and size, best'(q) in `best`)
    // ---- walk 2: the margin
    if (k.margin < 100u && cnt > 1u) {                                     // (wave-uniform)
        const double least = best.x * (double)(100u - k.margin);
        lo = 0xffffffffu; hi = 0; cnt = 0;
        list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
            uint32_t lf[GPL];
            if (!pot || !lane_map_row<GPL>(k.leaf, k.map_n, gl, lf)) return;
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j) {
                if (!((pot >> j) & 1u) || lf[j] == MK_NO_NODE) continue;
                const uint32_t g = gl + j;
                if (!(WalkBest::intersection(a, g, s[j]) * 100.0 >= least)) continue;
                lo = min(lo, g);
                hi = g;
                ++cnt;
            }
        });
        wave_span(lo, hi, cnt);
    }
    if (lane != 0) return;
    uint32_t node = MK_NO_NODE;
    if (cnt) {
        // ---- the climb: every node from leaf[lo] up holds lo; the first whose end lies beyond hi holds the whole list
        uint32_t v = k.leaf[lo];
        for (uint32_t step = 0; step <= k.depth && v != MK_NO_NODE && k.hi[v] <= hi; ++step) v = k.parent[v];
        mk_lca_tally *const t = k.tally + (v == MK_NO_NODE ? k.n_nodes : v);
        count(&t->reads, 1);
        count(&t->best_matches, best.m);
        count(&t->hits, cnt);
        node = v == MK_NO_NODE ? MK_LCA_ABOVE : v;
    }
    if (k.node) {
        const uint32_t at = k.q0 + qi;                                     // the query's place in its leaf, then in the set
        k.node[k.place ? k.place[at] : at] = node;
    }
}

}  // namespace

int launch_lca(mk_ctx *c, const LcaArgs &k)
{
    const char *missing = !k.tally ? "the lca pass needs the counters" : !k.leaf || !k.parent || !k.hi ? "the lca pass needs the taxonomy" : nullptr;
    return launch_walk(c, k.list, "lca counters", missing, [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(lca_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

}  // namespace mk
