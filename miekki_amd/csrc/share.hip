// K6i: ABUNDANCE BY EXPECTATION-MAXIMISATION over the reads that several genomes share -- a pool of per-read genome lists in
// device memory, filled by a sink on the list walk, and rounds over that pool that split every shared read among its genomes
// in proportion to the weights of the round before.  Integer sums only (include/miekki_hip.h, the share section).
//
//   collect: lca.hip's walks without a taxonomy.  Walk 1 finds best(q) and |L(q)| (walk_best.hpp); with a margin below 100
//            and more than one genome listed a second walk counts K(q), the genomes within the margin of the best.  |K| = 1 is
//            the best itself (it always passes its own margin, and a tie would be a second member): one add to unique[] from
//            lane 0.  |K| >= 2 leaves its size in count[q] and x* (100 - m) in least[q], the very double the second walk
//            compared with.  list.hip's scan turns the counts into places -- of the ids, and, with min(count, 1), of the
//            lists -- the host reads the chunk's two totals and grows the pool, and the write kernel walks the shared queries
//            once more: ids at exact offsets by a prefix sum over the wave, ascending, as list_kernel<true> writes its
//            records, one add to shared[g] per id.  A settled or unassigned query leaves the write kernel before its walk
//            (count[q] is wave-uniform).  A pass is therefore two walks per query at m = 100 and three at m < 100, for the
//            queries that several genomes share, against the tally's one.
//   round:   one launch over the pool.  The weight of genome g is read straight from the round before, (uint32_t)(prev[g] >>
//            shift) -- there is no normalising kernel -- the read's sum D is formed on chip, and every entry adds
//            floor((p << 32) / D) to next[g] with walk_best.hpp's count(): 64-bit, agent scope, relaxed, no return.  Lanes hold
//            CONSECUTIVE entries of a read, so a run of strains adds to contiguous words.  Two buffers ping-pong; the idle one
//            is seeded with unique << 32 by a kernel of its own on the stream.
//
// READS TO LANES.  Real lists are a family or less, so a wave per read would idle most lanes: a wave takes 64 / TEAM reads,
// one per team of TEAM consecutive lanes, D by a segmented xor-shuffle sum inside the team.  A read longer than TEAM takes the
// whole wave in a loop (sum pass, add pass; its ids and weights come from L2 the second time); the choice is per wave and
// wave-uniform: one long read among a wave's reads sends all of them through the loop, one after the other.  TEAM is 16 in
// the shipped library: measured best where the mapping shows at all (profiles/abundance.txt; MIEKKI_SHARE_TEAM = 8, 16, 32, 64
// picks another for tools/abundance_rate.py).  Pools of millions of short reads, us per round at TEAM 8 / 16 / 32 / 64: 4 M
// reads of 2 ids 232 / 278 / 551 / 1,078; 2 M of 4 ids 136 / 163 / 278 / 543; 1 M of 16 ids 285 / 146 / 172 / 280; 250 k of 64
// ids 104 / 106 / 106 / 110 (151 G ids/s) -- a wave per read costs up to 4 x on short lists, TEAM 8 twice on lists of 16.  The
// pool of the README's 20,000 reads (1.28 M ids at margin 100, 0.22 M at margin 10) is crossed in the time of a round's two
// launches, 9-19 us, where more waves hide more latency and TEAM 64 is 7-25 % ahead of 16: not what the choice was made for.
// Ungrouped ids -- a read's 64 adds in 64 different rows -- cost 4 x at any TEAM (62 us, 20 G ids/s): the adds bound it.
#include "walk_best.hpp"

namespace mk {

namespace {

// ---- collect ----------------------------------------------------------------------------------------------------------------
template <int SRC>
__global__ __launch_bounds__(256) void share_count_kernel(const ShareArgs k)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    const ListArgs &a = k.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;                                               // (wave-uniform: every lane of a wave reaches every shuffle)
    const uint32_t q = a.q_lo + qi;
    // ---- walk 1: the best of the listed genomes and their number
    WalkBest best;
    uint32_t cnt = 0;
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
        if (!pot) return;                                                  // (no shuffle in this sink: lanes may leave alone)
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) {
            if (!((pot >> j) & 1u)) continue;                              // (a set bit: gl + j < G)
            best.meet(a, gl + j, s[j]);
            ++cnt;
        }
    });
    best.wave_merge(cnt);                                                  // (now wave-uniform: |L(q)|, best(q) in `best`)
    // ---- walk 2: the margin
    double least = 0.0;
    if (k.margin < 100u && cnt > 1u) {                                     // (wave-uniform)
        least = best.x * (double)(100u - k.margin);
        cnt = 0;
        list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
            if (!pot) return;
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j)
                if (((pot >> j) & 1u) && WalkBest::intersection(a, gl + j, s[j]) * 100.0 >= least) ++cnt;
        });
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor(cnt, o);
    }
    if (lane != 0) return;
    if (cnt == 1u) {                                                       // settled: K(q) = { best(q) }
        count(k.unique + best.id, 1);
        count(k.settled, 1);
    }
    a.count[q] = cnt >= 2u ? cnt : 0u;
    k.least[q] = least;
}

template <int SRC>
__global__ __launch_bounds__(256) void share_write_kernel(const ShareArgs k)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    const ListArgs &a = k.list;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;
    const uint32_t q = a.q_lo + qi;
    const uint32_t n = a.count[q];
    if (n < 2u) return;                                                    // settled or unassigned (wave-uniform)
    const bool all = k.margin >= 100u;
    const double least = k.least[q];
    const uint64_t first = k.entries0 + a.rec_off[q];
    uint64_t at0 = first;                                                  // the wave's next id
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
        uint32_t keep = pot;
        if (!all && pot) {
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j)
                if (((pot >> j) & 1u) && !(WalkBest::intersection(a, gl + j, s[j]) * 100.0 >= least)) keep &= ~(1u << j);
        }
        if (__ballot(keep != 0) == 0) return;                              // wave-uniform
        const uint32_t m = __popc(keep);
        uint32_t incl = m;                                                 // ids of lanes 0 .. this one
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        uint64_t at = at0 + (incl - m);
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j)
            if ((keep >> j) & 1u) {
                k.ids[at++] = gl + j;
                count(k.shared + gl + j, 1);
            }
        at0 += (uint32_t)__shfl(incl, 63);
    });
    if (lane == 0) k.off[k.reads0 + k.read_off[q] + 1] = first + n;         // the list's end; its start is the end of the list before
}

// counters[ids[i]] += 1 for the lists the host brings (mk_share_add_lists)
__global__ __launch_bounds__(256) void share_bump_kernel(const uint32_t *__restrict__ ids, uint64_t n, uint64_t *counters)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) count(counters + ids[i], 1);
}

// ---- rounds -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, uint32_t o)
{
    return (uint64_t)(uint32_t)__shfl_xor((uint32_t)v, o) | ((uint64_t)(uint32_t)__shfl_xor((uint32_t)(v >> 32), o) << 32);
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, uint32_t from)
{
    return (uint64_t)(uint32_t)__shfl((uint32_t)v, from) | ((uint64_t)(uint32_t)__shfl((uint32_t)(v >> 32), from) << 32);
}

__device__ __forceinline__ uint32_t weight_of(const RoundArgs &k, uint32_t g) { return k.prev ? (uint32_t)(k.prev[g] >> k.shift) : 1u; }   // (p_0 = 1)
// what an entry of weight p gets of a read of `len` ids whose weights sum to D; a starved read is split evenly
__device__ __forceinline__ uint64_t share_of(uint32_t p, uint64_t D, uint64_t len) { return D ? ((uint64_t)p << 32) / D : 0x100000000ull / len; }

__global__ __launch_bounds__(256) void share_seed_kernel(const uint64_t *__restrict__ unique, uint32_t G, uint64_t *__restrict__ next)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < G) next[g] = unique[g] << 32;
}

template <uint32_t TEAM>
__global__ __launch_bounds__(256) void share_round_kernel(const RoundArgs k)
{
    constexpr uint32_t PER = 64u / TEAM;                                   // reads of a wave
    const uint32_t lane = threadIdx.x & 63u, team = lane / TEAM, tl = lane % TEAM;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * PER;
    if (r0 >= k.n_reads) return;                                           // (wave-uniform)
    const uint64_t r = r0 + team;
    uint64_t b = 0, len = 0;
    if (r < k.n_reads) { b = k.off[r]; len = k.off[r + 1] - b; }
    if (__ballot(len > TEAM) == 0) {
        // ---- a team per read: one entry per lane, D by a sum inside the team
        const bool has = tl < len;
        const uint32_t g = has ? k.ids[b + tl] : 0u;
        const uint32_t p = has ? weight_of(k, g) : 0u;
        uint64_t D = p;
#pragma unroll
        for (uint32_t o = 1; o < TEAM; o <<= 1) D += shfl_xor_u64(D, o);
        if (has) count(k.next + g, share_of(p, D, len));
        if (k.starved && tl == 0 && len && !D) count(k.starved, 1);
        return;
    }
    // ---- a long read among them: every read of the wave by all 64 lanes
    for (uint32_t t = 0; t < PER; ++t) {
        const uint64_t tb = shfl_u64(b, t * TEAM), tn = shfl_u64(len, t * TEAM);   // (wave-uniform)
        if (!tn) continue;
        uint64_t D = 0;
        for (uint64_t i = lane; i < tn; i += 64) D += weight_of(k, k.ids[tb + i]);
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) D += shfl_xor_u64(D, o);
        for (uint64_t i = lane; i < tn; i += 64) {
            const uint32_t g = k.ids[tb + i];
            count(k.next + g, share_of(weight_of(k, g), D, tn));
        }
        if (k.starved && lane == 0 && !D) count(k.starved, 1);
    }
}

// *delta += sum over g of |now[g] - before[g]| (before null: zeros)
__global__ __launch_bounds__(256) void share_delta_kernel(const uint64_t *__restrict__ now, const uint64_t *__restrict__ before, uint32_t G,
                                                          uint64_t *delta)
{
    __shared__ uint64_t part[4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    uint64_t d = 0;
    if (g < G) {
        const uint64_t x = now[g], y = before ? before[g] : 0;
        d = x > y ? x - y : y - x;
    }
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) d += shfl_xor_u64(d, o);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t sum = part[0] + part[1] + part[2] + part[3];
        if (sum) count(delta, sum);
    }
}

}  // namespace

int launch_share_count(mk_ctx *c, const ShareArgs &k)
{
    const char *missing = !k.unique || !k.settled || !k.list.count || !k.least ? "the share pass needs the pool's counters and the chunk's scratch" : nullptr;
    return launch_walk(c, k.list, "shared lists", missing, [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(share_count_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

int launch_share_write(mk_ctx *c, const ShareArgs &k)
{
    const char *missing = !k.shared || !k.ids || !k.off || !k.list.count || !k.list.rec_off || !k.read_off || !k.least ? "the share pass needs the pool and the chunk's places" : nullptr;
    return launch_walk(c, k.list, "shared lists", missing, [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL(share_write_kernel<decltype(src)::value>, grid, block, 0, c->stream, k);
    });
}

int launch_share_bump(mk_ctx *c, const uint32_t *d_ids, uint64_t n, uint64_t *d_counters)
{
    if (!n) return MK_OK;
    if (n > 0x7fffffffull * 256) { set_error("too many ids for one launch"); return MK_ERR_ARG; }
    hipLaunchKernelGGL(share_bump_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, d_ids, n, d_counters);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int share_team(uint32_t *team)
{
    *team = 16;
    if (const char *e = getenv("MIEKKI_SHARE_TEAM")) {
        const long v = atol(e);
        if (v != 8 && v != 16 && v != 32 && v != 64) { set_error("MIEKKI_SHARE_TEAM takes 8, 16, 32 or 64: %s", e); return MK_ERR_ARG; }
        *team = (uint32_t)v;
    }
    return MK_OK;
}

int launch_share_seed(mk_ctx *c, const uint64_t *d_unique, uint32_t G, uint64_t *d_next)
{
    if (!G) return MK_OK;
    hipLaunchKernelGGL(share_seed_kernel, dim3((G + 255) / 256), dim3(256), 0, c->stream, d_unique, G, d_next);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_share_round(mk_ctx *c, const RoundArgs &k, uint32_t team)
{
    if (!k.n_reads) return MK_OK;
    const uint64_t per_block = 4ull * (64u / team), blocks = (k.n_reads + per_block - 1) / per_block;
    if (blocks > 0x7fffffffull) { set_error("too many shared reads for one launch"); return MK_ERR_ARG; }
    const dim3 grid((uint32_t)blocks), block(256);
    switch (team) {
    case 8: hipLaunchKernelGGL(share_round_kernel<8>, grid, block, 0, c->stream, k); break;
    case 16: hipLaunchKernelGGL(share_round_kernel<16>, grid, block, 0, c->stream, k); break;
    case 32: hipLaunchKernelGGL(share_round_kernel<32>, grid, block, 0, c->stream, k); break;
    default: hipLaunchKernelGGL(share_round_kernel<64>, grid, block, 0, c->stream, k); break;
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_share_delta(mk_ctx *c, const uint64_t *d_now, const uint64_t *d_before, uint32_t G, uint64_t *d_delta)
{
    if (!G) return MK_OK;
    hipLaunchKernelGGL(share_delta_kernel, dim3((G + 255) / 256), dim3(256), 0, c->stream, d_now, d_before, G, d_delta);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
