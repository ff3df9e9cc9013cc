// K6f: the profile of a read set -- per genome, how many queries list it, list it alone, have it as their best hit, and the
// matches of those -- as four 64-bit counters per genome in device memory.
//
//   tally:   list_kernel's walk (list_walk.hpp: one wave per query over the chunk's scores or partial counts, the f32 screen,
//            the double decision) with a counting sink: a passing (query, genome) pair is not written anywhere, the genome's
//            `listed` grows by one and the lane keeps the best pair it has met; after the walk the wave agrees on the query's
//            number of listed genomes and on its best one, and lane 0 adds the query to that genome's counters.
//
// best(q), its tie rule and the adds to the counters (64-bit, agent scope, relaxed, no return) are walk_best.hpp's, which
// clade.hip and lca.hip share: WalkBest, count().  No LDS, nothing waits for another wave.
#include "walk_best.hpp"

namespace mk {

namespace {

template <int SRC>
__global__ __launch_bounds__(256) void tally_kernel(const TallyArgs k)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    const ListArgs &a = k.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;                                               // (wave-uniform: every lane of a wave reaches every shuffle)
    const uint32_t q = a.q_lo + qi;
    mk_tally *const t = k.tally;
    WalkBest best;                                                         // this lane's listed genomes, and the best of them
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) {
            if (!((pot >> j) & 1u)) continue;                              // (a set bit: gl + j < G)
            const uint32_t g = gl + j;
            count(&t[g].listed, 1);
            best.meet(a, g, s[j]);
        }
    });
    uint32_t total = best.n;                                               // the query's listed genomes, once summed
    best.wave_merge(total);
    if (lane == 0 && total) {
        count(&t[best.id].best, 1);
        count(&t[best.id].best_matches, best.m);
        if (total == 1) count(&t[best.id].unique, 1);
    }
}

}  // namespace

int launch_tally(mk_ctx *c, const TallyArgs &k)
{
    return launch_walk(c, k.list, "tallies", k.tally ? nullptr : "the tally pass needs the counters", [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(tally_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

}  // namespace mk
