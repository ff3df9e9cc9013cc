// K6i: greedy gather -- which few indexed genomes, taken together, explain a sample (sourmash's `gather`: the greedy minimum
// set cover over the cover table of cover.hip).
//
//   live_0       = seen
//   rem_r(g)     #{ p : column_g[p] != empty and live_r(p, column_g[p]) }; rem_0 = covered
//   round r:     w_r = the genome of largest rem_r, the smallest id among equals: the 64-bit key rem << 32 | ~id, maximised.
//                Stop when rem_r(w_r) < min_new, or when r == max_picks != 0.  Otherwise fresh = rem_r(w_r), and live_{r+1} is
//                live_r without the cells (p, column_w[p]) that were live.
//   depth_sum    the sum of mult(p, v) over the cells the pick struck (depth.hip's byte table), 0 without a table
// Integers only: the picks are a function of the table, the matrix, min_new and max_picks.
//
// A round is three kernels on the context's stream, and rounds are queued without a host wait in between:
//   pick:    arg-max of the key over rem[0 .. G): lanes stride over the genomes, a wave reduces by shuffles, a workgroup through
//            LDS, and one 64-bit agent-scope atomic max per workgroup goes into the round's slot (zero: nobody yet -- the key of
//            genome 0 with rem 0 is 2^32 - 1, so a slot that was written is never zero).
//   take:    one lane per partition.  The slot names the winner w and fresh.  fresh < min_new, or the cap reached: the `done`
//            flag is set and everybody returns -- as does every kernel of every later round.  Otherwise the lane reads
//            v = column_w[p] where row p lies (mat_row: one sector per row, P sectors a round), and a v != empty whose bit is
//            live is cleared -- a plain load in front, then an agent-scope atomic and-not whose RETURN says whether this lane
//            cleared it (a partition's slice is at least 8 words, so no two lanes share a word; the atomic stays, as mark's or
//            does) -- and appended as (p, v) to the round's strike list: one atomic add per wave on the pick record's counter,
//            lanes placed by the ballot.  With a depth table the struck cells' bytes are summed per wave into the record.
//   strike:  a fixed grid; the list's length is read from the record, never by the host.  Waves stride over items of (list
//            entry, run of 8 tiles of 1 KiB).  A lane loads 16 bytes of row p, the next tile's load in flight, and tests each
//            dword for a byte (halfword) equal to the wave-uniform v with one xor and the has-zero trick; matches are rare
//            (G / 256 per row at one byte, a family's members at two), and only a dword that has one is taken apart.  Every
//            match at a column g < G is one relaxed agent-scope subtraction of 1 from rem[g] -- columns [G, pitch) are zero
//            padding and equal v = 0, the trap table_pass_kernel names.  The winner's own column matches in every struck
//            row: its rem ends at 0, and it is never picked again.
//   recount: (MIEKKI_GATHER_RECOUNT=1) instead of strike: rem zeroed and counted again by cover.hip's count pass over the
//            struck table.  The count pass does not look at `done`, so this route waits for the host after every round unless
//            MIEKKI_GATHER_ROUNDS says otherwise.
#include <algorithm>
#include <cstdlib>

#include "mk_internal.hpp"

namespace mk {

namespace {

constexpr uint32_t kStrikeRun = 8;        // tiles of a row per strike item

__device__ __forceinline__ bool is_done(const uint32_t *done) { return __hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; }

__global__ __launch_bounds__(256) void gather_pick_kernel(const uint32_t *__restrict__ rem, uint32_t G, const uint32_t *__restrict__ done,
                                                          unsigned long long *__restrict__ slot)
{
    __shared__ unsigned long long s_best[4];
    if (is_done(done)) return;                                             // (uniform over the launch: set by an earlier kernel)
    unsigned long long best = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < G; g += (uint64_t)gridDim.x * 256u)
        best = max(best, ((unsigned long long)rem[g] << 32) | (uint32_t)~(uint32_t)g);
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, o));
    if ((threadIdx.x & 63u) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        best = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
        if (best) (void)__hip_atomic_fetch_max(slot, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// rec->covered counts the list's entries (the host compares it with fresh and then puts rem_0 there)
template <int W>
__global__ __launch_bounds__(256) void gather_take_kernel(MatRef M, uint64_t ld, uint32_t P, uint32_t round, uint32_t cap, uint32_t min_new,
                                                          const unsigned long long *__restrict__ slot, uint32_t *__restrict__ live,
                                                          const uint8_t *__restrict__ mult, uint32_t *__restrict__ done, mk_pick *__restrict__ rec,
                                                          uint64_t *__restrict__ list)
{
    constexpr uint32_t kBits = 8 * W, kEmpty = (1u << kBits) - 1u;
    if (is_done(done)) return;
    const unsigned long long key = *slot;
    const uint32_t fresh = (uint32_t)(key >> 32), w = ~(uint32_t)key;
    if (round >= cap || fresh < min_new) {                                 // (every workgroup decides alike; one says so)
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const uint32_t p = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool hit = false;
    uint32_t v = 0;
    uint64_t cell = 0;
    if (p < P) {
        const uint8_t *row = mat_row(M, p, ld);
        v = W == 1 ? (uint32_t)row[w] : (uint32_t)reinterpret_cast<const uint16_t *>(row)[w];
        if (v != kEmpty) {
            cell = ((uint64_t)p << kBits) + v;
            uint32_t *word = live + (cell >> 5);
            const uint32_t m = 1u << ((uint32_t)cell & 31u);
            if (*word & m) hit = (__hip_atomic_fetch_and(word, ~m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m) != 0;
        }
    }
    const unsigned long long mask = __ballot(hit);
    if (mask) {                                                            // (uniform over the wave)
        uint32_t base = 0;
        if (lane == 0) base = __hip_atomic_fetch_add(&rec->covered, (uint32_t)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = __shfl(base, 0);
        if (hit) list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint64_t)p | ((uint64_t)v << 32);   // (base + place < fresh <= P)
        if (mult) {
            unsigned long long sum = hit ? mult[cell] : 0u;
#pragma unroll
            for (uint32_t o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            if (lane == 0 && sum)
                (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(&rec->depth_sum), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { rec->genome = w; rec->fresh = fresh; }
}

template <int W>
__global__ __launch_bounds__(256) void gather_strike_kernel(MatRef M, uint64_t ld, uint32_t G, uint32_t ntiles, uint32_t runs,
                                                            const uint32_t *__restrict__ done, const mk_pick *__restrict__ rec,
                                                            const uint64_t *__restrict__ list, uint32_t *__restrict__ rem)
{
    constexpr uint32_t kBits = 8 * W, kMask = (1u << kBits) - 1u, kPerWord = 4u / W, kPerLane = 16u / W;
    constexpr uint32_t kOnes = W == 1 ? 0x01010101u : 0x00010001u, kHigh = kOnes << (kBits - 1u);
    if (is_done(done)) return;                                             // (this round's take step may have set it)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t items = (uint64_t)rec->covered * runs, nwaves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); it < items; it += nwaves) {
        const uint64_t ent = list[it / runs];                              // (uniform)
        const uint32_t p = (uint32_t)ent, vv = (uint32_t)(ent >> 32) * kOnes;
        const uint32_t t0 = (uint32_t)(it % runs) * kStrikeRun, t1 = min(ntiles, t0 + kStrikeRun);
        const uint8_t *row = mat_row(M, p, ld) + lane * 16u;               // (ld covers whole tiles: launch_gather_round checks)
        uint4 cur = *reinterpret_cast<const uint4 *>(row + (uint64_t)t0 * kTileBytes), nxt = cur;
        for (uint32_t t = t0; t < t1; ++t) {
            if (t + 1 < t1) nxt = *reinterpret_cast<const uint4 *>(row + (uint64_t)(t + 1) * kTileBytes);
            const uint32_t x[4] = {cur.x, cur.y, cur.z, cur.w};
            const uint32_t g0 = t * (kTileBytes / W) + lane * kPerLane;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t d = x[k] ^ vv;
                if (!((d - kOnes) & ~d & kHigh)) continue;                 // no byte (halfword) of d is zero: no fingerprint equals v
#pragma unroll
                for (uint32_t j = 0; j < kPerWord; ++j) {
                    const uint32_t g = g0 + k * kPerWord + j;
                    if (((d >> (j * kBits)) & kMask) == 0 && g < G)        // (columns [G, pitch) are padding and equal v = 0)
                        (void)__hip_atomic_fetch_sub(rem + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            cur = nxt;
        }
    }
}

}  // namespace

// MIEKKI_GATHER_RECOUNT=1: the count pass over the struck table instead of the strike step (tools/gather_rate.py measures both)
bool gather_recount()
{
    if (const char *e = getenv("MIEKKI_GATHER_RECOUNT")) return atol(e) != 0;
    return false;
}

// Rounds queued per host wait: 32 (the recount route: 1), unless MIEKKI_GATHER_ROUNDS says otherwise
uint32_t gather_rounds_per_wait()
{
    if (const char *e = getenv("MIEKKI_GATHER_ROUNDS")) { const long v = atol(e); if (v >= 1) return (uint32_t)std::min<long>(v, 1 << 20); }
    return gather_recount() ? 1u : 32u;
}

// One round, queued on c->stream.  Raw cold rows.  a.slots and a.recs are the arrays' bases; everything was zeroed before round 0.
int launch_gather_round(mk_ctx *c, const GatherArgs &a, uint32_t round)
{
    const uint32_t G = c->G, P = c->P;
    uint32_t ntiles = 0;
    MK_TRY(row_tiles(c, &ntiles));
    const dim3 block(256);
    const uint32_t pick_blocks = (uint32_t)std::min<uint64_t>(1024, ((uint64_t)G + 255) / 256);
    hipLaunchKernelGGL(gather_pick_kernel, dim3(pick_blocks), block, 0, c->stream, a.rem, G, a.done, a.slots + round);
    const dim3 take_grid((P + 255) / 256);
    mk_pick *rec = a.recs + round;
    if (c->W == 1) hipLaunchKernelGGL(gather_take_kernel<1>, take_grid, block, 0, c->stream, mat_ref(c), c->ld, P, round, a.cap, a.min_new, a.slots + round, a.live, a.mult, a.done, rec, a.list);
    else hipLaunchKernelGGL(gather_take_kernel<2>, take_grid, block, 0, c->stream, mat_ref(c), c->ld, P, round, a.cap, a.min_new, a.slots + round, a.live, a.mult, a.done, rec, a.list);
    MK_HIP(hipGetLastError());
    if (a.recount) {
        MK_HIP(hipMemsetAsync(a.rem, 0, (size_t)G * 4, c->stream));
        return launch_cover_count(c, a.live, a.rem, nullptr);
    }
    // a list holds at most P entries: as many waves as that takes, 2,048 workgroups at the most
    const uint32_t runs = (ntiles + kStrikeRun - 1) / kStrikeRun;
    const uint32_t strike_blocks = (uint32_t)std::min<uint64_t>(2048, ((uint64_t)P * runs + 3) / 4);
    if (c->W == 1) hipLaunchKernelGGL(gather_strike_kernel<1>, dim3(strike_blocks), block, 0, c->stream, mat_ref(c), c->ld, G, ntiles, runs, a.done, rec, a.list, a.rem);
    else hipLaunchKernelGGL(gather_strike_kernel<2>, dim3(strike_blocks), block, 0, c->stream, mat_ref(c), c->ld, G, ntiles, runs, a.done, rec, a.list, a.rem);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
