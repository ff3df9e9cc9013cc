// The pieces every COUNTING sink on the list walk shares (tally.hip, clade.hip, lca.hip): the add to a counter, a query's best
// hit -- per lane along the walk, then agreed on by the wave -- and a lane's entries of a per-genome map.  All of it is inlined
// into the sink's kernel: no memory traffic of its own, no LDS, nothing waits for another wave.
#pragma once
#include "list_walk.hpp"

namespace mk {

// The counters.  Integer sums only, so the result does not depend on the order of the adds: chunks, schedules and launch order
// leave no trace.  Waves on every XCD add to the same words and the per-XCD L2s are not coherent, so -- as for family.hip's
// forest -- every add is an agent-scope atomic; relaxed, because nothing in a sink READS a counter or orders anything by one:
// the result of an add is not used (the no-return form), and the counters are read only by later launches or copies on the
// stream.
__device__ __forceinline__ void count(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// best(q) is the single hit of filter_results(row, 1, ...) (Miekki.cpp:376-397): a heap of one is replaced unless
// front.intersection > intersection (387), so the largest intersection wins and, among equal ones, the genome met last: the
// largest id.  A lane meets its genomes in ascending id and replaces with the reference's own test; lanes are merged by the
// lexicographic maximum of (intersection, id), the intersection compared as the double the reference computes (382-383).
struct WalkBest {
    uint32_t n = 0, id = 0, m = 0;                                         // the genomes met; the best of them and its matches
    double x = 0.0;                                                        // ... and its intersection

    // Miekki.cpp:382-383, in the double operations with which the walk decided that the pair passes
    static __device__ __forceinline__ double intersection(const ListArgs &a, uint32_t g, uint32_t s)
    {
        const double jac = (double)s / (double)a.sketch_size[g];
        return jac * (double)a.genome_size[g];
    }

    // this lane meets genome g with s matches (in ascending id)
    __device__ __forceinline__ void meet(const ListArgs &a, uint32_t g, uint32_t s)
    {
        const double inter = intersection(a, g, s);
        if (n == 0 || !(x > inter)) { x = inter; id = g; m = s; }          // Miekki.cpp:387: ties replace -- ascending id here
        ++n;
    }

    // after the walk: every lane gets the wave's best (n != 0: there is one) and, on the same steps, the sum over the lanes of
    // a count of the sink's, `sum` (a sink without one brings a zero it does not read).  All 64 lanes call it.
    __device__ __forceinline__ void wave_merge(uint32_t &sum)
    {
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) {
            sum += (uint32_t)__shfl_xor(sum, o);
            const uint32_t on = (uint32_t)__shfl_xor(n, o), oid = (uint32_t)__shfl_xor(id, o), om = (uint32_t)__shfl_xor(m, o);
            const double ox = __hiloint2double(__shfl_xor(__double2hiint(x), o), __shfl_xor(__double2loint(x), o));
            if (on && (!n || ox > x || (ox == x && oid > id))) { n = on; x = ox; id = oid; m = om; }   // (387 across lanes: a tie to the largest id)
        }
    }
};

// A lane's GPL entries map[gl ..] of a per-genome map that is padded to whole tiles (as the size arrays are: the loads are
// whole) into out[]; false: the lane's genomes are beyond the map's map_n entries -- left out.
template <uint32_t GPL>
__device__ __forceinline__ bool lane_map_row(const uint32_t *map, uint32_t map_n, uint32_t gl, uint32_t (&out)[GPL])
{
    if (gl >= map_n) return false;
    const uint4 c0 = *reinterpret_cast<const uint4 *>(map + gl);
    out[0] = c0.x; out[1] = c0.y; out[2] = c0.z; out[3] = c0.w;
    if constexpr (GPL == 8) {
        const uint4 c1 = *reinterpret_cast<const uint4 *>(map + gl + 4);
        out[4] = c1.x; out[5] = c1.y; out[6] = c1.z; out[7] = c1.w;
    }
    return true;
}

}  // namespace mk
