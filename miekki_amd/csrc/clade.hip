// K6g: the profile of a read set by CLADE -- per group of genomes, how many queries list a member, list members of it only,
// have their best hit in it, the matches of those, and the (query, member) pairs -- as five 64-bit counters per clade in
// device memory.
//
//   clade tally:  tally.hip's walk with one more array, clade[g] = the clade number of local genome g or MK_NO_CLADE (left
//                 out: the genome is not there for this pass).  A passing pair is not written anywhere.  The best hit, the
//                 load of a lane's map entries and the add to a counter are walk_best.hpp's, shared with tally.hip and lca.hip.
//
// Deduplication without memory.  `listed` counts a query ONCE per clade, however many members it lists.  The map's numbers
// are non-decreasing along the ids (mk_clade_map_create refuses any other) and the walk meets ids in ascending order, so a
// passing genome is the FIRST of its clade for this query exactly when the nearest passing genome with a clade to its left
// carries another number -- and, the sequence being non-decreasing, that neighbour's number is the maximum over everything to
// the left (an exclusive prefix maximum of "last passing clade + 1", 0 = none).  Because it is the NEAREST one, the prefix
// maximum over the 64 lanes needs no scan: a ballot of the lanes that hold a passing clade, the highest set bit below the
// lane, one __shfl from that lane.  Inside a lane neighbours among its GPL genomes are compared; across steps the value of
// the highest such lane is carried, wave-uniform.  Steps in which the ballot is zero -- most steps of most reads -- cost a
// ballot and a uniform branch more than they cost tally_kernel.  No LDS, no scratch, no capacity: a read that lists every
// genome is a read like any other.
//
// best'(q) is walk_best.hpp's best(q) over the genomes that have a clade: a left-out genome never becomes a lane's best.  The sum
// of the first-of-clade flags over the wave is the number of distinct clades the query lists: 1 = unique.
//
// The counters are added to by walk_best.hpp's count() (64-bit, agent scope, relaxed, no return).  `hits` gets one add
// per run of consecutive passing members of one clade in a step of the wave, summed over the lanes from ballots: with one add
// per LANE and run, reads of one family put 12 adds each on one 40-byte row of counters and the walk took 4.0 ms where the
// plain tally takes 1.4 (profiles/clade_tally.txt); with one per wave it takes 1.1.
#include "walk_best.hpp"

namespace mk {

namespace {

template <int SRC>
__global__ __launch_bounds__(256) void clade_kernel(const CladeArgs k)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    const ListArgs &a = k.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;                                               // (wave-uniform: every lane of a wave reaches every shuffle)
    const uint32_t q = a.q_lo + qi;
    mk_clade_tally *const t = k.tally;
    const uint64_t below_me = (1ull << lane) - 1ull;
    WalkBest best;                                                         // this lane's listed genomes with a clade, and the best of them
    uint32_t firsts = 0;                                                   // first-of-clade genomes this lane has met
    uint32_t carry = 0;                                                    // wave-uniform: the last passing clade + 1 of the steps before, 0 = none
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
        uint32_t cl[GPL], last = 0;                                        // last: this lane's last passing clade + 1 of this step
        // (genomes beyond the map are left out; the bound is tested here too: behind lane_map_row's own test alone the compiler
        // lays this step out 5 % longer, with it the kernel has the size and the registers it had before the helper)
        if (pot && gl < k.map_n && lane_map_row<GPL>(k.clade, k.map_n, gl, cl)) {
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j)
                if (((pot >> j) & 1u) && cl[j] != MK_NO_CLADE) last = cl[j] + 1u;
                else pot &= ~(1u << j);                                    // (left out: not listed in this pass)
        } else {
            pot = 0;
        }
        const uint64_t have = __ballot(last != 0);
        if (!have) return;                                                 // (wave-uniform)
        const uint64_t left_of_me = have & below_me;
        const uint32_t from = left_of_me ? 63u - (uint32_t)__clzll((long long)left_of_me) : lane;
        const uint32_t left_last = (uint32_t)__shfl((int)last, (int)from); // the nearest lane to the left that lists a clade ...
        uint32_t prev = left_of_me ? left_last : carry;                    // ... or the steps before
        carry = (uint32_t)__shfl((int)last, (int)(63u - (uint32_t)__clzll((long long)have)));
        uint32_t run = 0, run_c = 0;                                       // consecutive passing members of clade run_c
        uint32_t runs = 0, head_c = 0, head_n = 0;                         // the runs that have ended, the first of them
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) {
            if (!((pot >> j) & 1u)) continue;                              // (a set bit: gl + j < G, and a clade)
            const uint32_t g = gl + j, c = cl[j];
            if (run && c != run_c) {
                if (!runs) { head_c = run_c; head_n = run; }       // (the lane's first run may go on from the lane to its left)
                else count(&t[run_c].hits, run);
                ++runs;
                run = 0;
            }
            if (c + 1u != prev) { count(&t[c].listed, 1); ++firsts; prev = c + 1u; }
            run_c = c;
            ++run;
            best.meet(a, g, s[j]);
        }
        // `hits`: one add per run of the WAVE's step.  A lane that lists a clade has a first run (head) and a last one (tail:
        // run_c, run) -- the same run where it lists one clade only; runs in between were added above.  The head JOINS the tail
        // of the nearest such lane to the left when the clades are equal.  A tail that is not a joined head STARTS a run of the
        // wave, and the lanes up to the next start that join are its own: their heads' lengths (at most GPL <= 8: four bits)
        // are summed from ballots of their bits -- no scan.
        const bool mine = last != 0, one_clade = runs == 0;
        if (one_clade) { head_c = run_c; head_n = run; }
        const bool joins = mine && left_of_me && left_last == head_c + 1u;
        const bool starts = mine && (!one_clade || !joins);
        const uint64_t start_lanes = __ballot(starts);
        uint64_t bit[4];
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) bit[b] = __ballot(joins && ((head_n >> b) & 1u));
        if (mine && !one_clade && !joins) count(&t[head_c].hits, head_n);  // a head that no tail goes on into
        if (starts) {
            const uint64_t above_me = ~((2ull << lane) - 1ull), later = start_lanes & above_me;
            const uint32_t next = later ? (uint32_t)__builtin_ctzll(later) : 63u;    // (a start that joins: its head is this run's end)
            const uint64_t range = ((2ull << next) - 1ull) & above_me;
            uint32_t sum = run;
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b) sum += (uint32_t)__popcll(bit[b] & range) << b;
            count(&t[run_c].hits, sum);
        }
    });
    uint32_t clades = firsts;                                              // the distinct clades the query lists, once summed
    best.wave_merge(clades);
    if (lane == 0 && clades) {
        const uint32_t c = k.clade[best.id];                               // (the best one carries a clade: it was listed)
        count(&t[c].best, 1);
        count(&t[c].best_matches, best.m);
        if (clades == 1) count(&t[c].unique, 1);
    }
}

}  // namespace

int launch_clade_tally(mk_ctx *c, const CladeArgs &k)
{
    const char *missing = !k.tally ? "the clade pass needs the counters" : !k.clade ? "the clade pass needs the map" : nullptr;
    return launch_walk(c, k.list, "clade tallies", missing, [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(clade_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

}  // namespace mk
