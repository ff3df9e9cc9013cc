// K6f: the profile of a read set -- per genome, how many queries list it, list it alone, have it as their best hit, and the
// matches of those -- as four 64-bit counters per genome in device memory.
//
//   tally:   list_kernel's walk (list_walk.hpp: one wave per query over the chunk's scores or partial counts, the f32 screen,
//            the double decision) with a counting sink: a passing (query, genome) pair is not written anywhere, the genome's
//            `listed` grows by one and the lane keeps the best pair it has met; after the walk the wave agrees on the query's
//            number of listed genomes and on its best one, and lane 0 adds the query to that genome's counters.
//
// best(q) is the single hit of filter_results(row, 1, ...) (Miekki.cpp:376-397): a heap of one is replaced unless
// front.intersection > intersection (387), so the largest intersection wins and, among equal ones, the genome met last: the
// largest id.  A lane meets its genomes in ascending id and replaces with the reference's own test; lanes are merged by the
// lexicographic maximum of (intersection, id), the intersection compared as the double the reference computes (382-383).
//
// The counters.  Integer sums only, so the result does not depend on the order of the adds: chunks, schedules and launch order
// leave no trace.  Waves on every XCD add to the same words and the per-XCD L2s are not coherent, so -- as for family.hip's
// forest -- every add is an agent-scope atomic; relaxed, because nothing here READS a counter or orders anything by one: the
// result of an add is not used (the no-return form), and the counters are read only by later launches or copies on the
// stream.  No LDS, nothing waits for another wave.
#include "list_walk.hpp"

namespace mk {

namespace {

__device__ __forceinline__ void count(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

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
    uint32_t n = 0, id = 0, m = 0;                                         // this lane's listed genomes, and the best of them
    double x = 0.0;
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) {
            if (!((pot >> j) & 1u)) continue;                              // (a set bit: gl + j < G)
            const uint32_t g = gl + j;
            count(&t[g].listed, 1);
            const double jac = (double)s[j] / (double)a.sketch_size[g];    // Miekki.cpp:382-383, as the walk decided it
            const double inter = jac * (double)a.genome_size[g];
            if (n == 0 || !(x > inter)) { x = inter; id = g; m = s[j]; }   // Miekki.cpp:387: ties replace -- ascending id here
            ++n;
        }
    });
    uint32_t total = n;
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) {
        total += (uint32_t)__shfl_xor(total, o);
        const uint32_t on = (uint32_t)__shfl_xor(n, o), oid = (uint32_t)__shfl_xor(id, o), om = (uint32_t)__shfl_xor(m, o);
        const double ox = __hiloint2double(__shfl_xor(__double2hiint(x), o), __shfl_xor(__double2loint(x), o));
        if (on && (!n || ox > x || (ox == x && oid > id))) { n = on; x = ox; id = oid; m = om; }
    }
    if (lane == 0 && total) {
        count(&t[id].best, 1);
        count(&t[id].best_matches, m);
        if (total == 1) count(&t[id].unique, 1);
    }
}

}  // namespace

int launch_tally(mk_ctx *c, const TallyArgs &k)
{
    return launch_walk(c, k.list, "tallies", k.tally ? nullptr : "the tally pass needs the counters", [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(tally_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

int launch_tally_reset(mk_ctx *c, mk_tally *d_tally, uint32_t n)
{
    if (!n) return MK_OK;
    MK_HIP(hipMemsetAsync(d_tally, 0, (size_t)n * sizeof(mk_tally), c->stream));
    return MK_OK;
}

}  // namespace mk
