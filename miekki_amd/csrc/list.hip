// K6c: Miekki::filter_results (Miekki.cpp:376-397) for any nresults -- every genome above the thresholds when nresults is
// the index size -- for whole query sets on the device.
//
// select_kernel (K6) keeps its top-N multiset one value per lane and merge_kernel (K6b) its heap in a per-lane array, which is
// what bounds them to 64 results.  Here nothing is bounded by a register file:
//   1. count:   one wave per query walks the chunk's scores (plain / dense schedule) or per-range partial counts (slab
//               schedule) exactly as the selection does and counts the genomes that pass min_score and min_intersection
//               (381-384), the latter decided in the reference's double operations behind an f32 screen;
//   2. scan:    exclusive scans of the counts (record offsets) and of min(count, nresults) (result offsets);
//   3. write:   the same walk again, now writing genome | matches << 32 at the exact offsets: within a step the lanes' places
//               come from a prefix sum over the wave of how many genomes each lane passes, lanes hold consecutive genomes, and
//               the steps ascend -- so a query's records are in ascending genome id, the order filter_results meets them in,
//               with no atomics anywhere;
//   4. heap:    one lane per query replays the reference's heap over its records -- libstdc++'s __push_heap / __adjust_heap
//               restated as in merge.hip, over (key, ref) pairs in global memory, min(nresults, count) + 1 per query --
//               and gathers the hits: ties fall as the host's own std:: calls let them fall (mk_filter_candidates).
// The host (api_query.hip: qset_run_list) sizes the buffers from the scans and cuts a chunk whose records exceed the budget
// into runs of fewer queries, written from the scores / partials the chunk's ONE scan left.
#include "list_walk.hpp"

namespace mk {

namespace {

// Genomes of query q (of the chunk) that pass both thresholds: counted (WRITE = false) or written as records.  The walk
// and the decision are list_walk's (list_walk.hpp); SRC as there.
template <int SRC, bool WRITE>
__global__ __launch_bounds__(256) void list_kernel(const ListArgs a)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t qi = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (qi >= a.q_n) return;
    const uint32_t q = a.q_lo + qi;
    uint32_t total = 0;                                                  // (count pass) this lane's
    uint64_t at0 = WRITE ? a.rec_off[q] - a.rec_off[a.q_lo] : 0;          // (write pass) the wave's next record
    list_walk<SRC>(a, q, lane, [&](uint32_t gl, const uint32_t (&s)[GPL], uint32_t pot) {
        if constexpr (!WRITE) {
            total += __popc(pot);
        } else {
            if (__ballot(pot != 0) == 0) return;                            // wave-uniform
            const uint32_t n = __popc(pot);
            uint32_t incl = n;                                              // records of lanes 0 .. this one
#pragma unroll
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            uint64_t at = at0 + (incl - n);
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j)
                if ((pot >> j) & 1u) a.rec[at++] = (uint64_t)(gl + j + a.genome_id_base) | ((uint64_t)s[j] << 32);
            at0 += (uint32_t)__shfl(incl, 63);
        }
    });
    if constexpr (!WRITE) {
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
        if (lane == 0) a.count[q] = total;
    }
}

// rec_off = exclusive scan of count, res_off = exclusive scan of min(count, nresults): one workgroup, a run of queries per lane
__global__ __launch_bounds__(1024) void list_scan_kernel(const uint32_t *__restrict__ count, uint32_t n, uint32_t nresults,
                                                         uint64_t *__restrict__ rec_off, uint64_t *__restrict__ res_off)
{
    __shared__ uint64_t sa[1024], sb[1024];
    const uint32_t tid = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
    uint64_t a = 0, b = 0;
    for (uint32_t i = lo; i < hi; ++i) { a += count[i]; b += min(count[i], nresults); }
    sa[tid] = a; sb[tid] = b;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t ua = tid >= o ? sa[tid - o] : 0, ub = tid >= o ? sb[tid - o] : 0;
        __syncthreads();
        sa[tid] += ua; sb[tid] += ub;
        __syncthreads();
    }
    uint64_t ea = sa[tid] - a, eb = sb[tid] - b;
    for (uint32_t i = lo; i < hi; ++i) {
        rec_off[i] = ea; res_off[i] = eb;
        ea += count[i]; eb += min(count[i], nresults);
    }
    if (tid == 1023) { rec_off[n] = sa[1023]; res_off[n] = sb[1023]; }
}

// ---- the heap of filter_results over a query's records, in global memory (merge.hip's operations, same names)
struct HeapMem {
    double *__restrict__ key;
    uint32_t *__restrict__ ref;
};

// comp(a, b) of the reference's priority queue: a.intersection > b.intersection
__device__ __forceinline__ bool heap_comp(double a, double b) { return a > b; }

// std::__push_heap(first, hole, top, value, comp)
__device__ __forceinline__ void sift_up(const HeapMem &h, int64_t hole, int64_t top, double vkey, uint32_t vref)
{
    int64_t parent = (hole - 1) / 2;
    while (hole > top && heap_comp(h.key[parent], vkey)) {
        h.key[hole] = h.key[parent]; h.ref[hole] = h.ref[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    h.key[hole] = vkey; h.ref[hole] = vref;
}

// std::__adjust_heap(first, hole, len, value, comp)
__device__ __forceinline__ void adjust(const HeapMem &h, int64_t hole, int64_t len, double vkey, uint32_t vref)
{
    const int64_t top = hole;
    int64_t child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if (heap_comp(h.key[child], h.key[child - 1])) --child;
        h.key[hole] = h.key[child]; h.ref[hole] = h.ref[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        h.key[hole] = h.key[child - 1]; h.ref[hole] = h.ref[child - 1];
        hole = child - 1;
    }
    sift_up(h, hole, top, vkey, vref);
}

// std::pop_heap on [0, len): the front moves to slot len-1, the rest is a heap again
__device__ __forceinline__ void pop_to_back(const HeapMem &h, int64_t len)
{
    if (len <= 1) return;
    const double vkey = h.key[len - 1];
    const uint32_t vref = h.ref[len - 1];
    h.key[len - 1] = h.key[0]; h.ref[len - 1] = h.ref[0];
    adjust(h, 0, len - 1, vkey, vref);
}

// jaccard and intersection of a record in the reference's double operations (Miekki.cpp:382-383): the two operations the
// write pass decided with, so the keys are bit-identical to what the thresholds saw
__device__ __forceinline__ mk_hit hit_of(uint64_t rec, const uint32_t *__restrict__ ss, const uint64_t *__restrict__ gs, uint32_t id_base)
{
    const uint32_t g = (uint32_t)rec - id_base;
    mk_hit o;
    o.genome = (uint32_t)rec;
    o.matches = (uint32_t)(rec >> 32);
    o.jaccard = (double)o.matches / (double)ss[g];
    o.intersection = o.jaccard * (double)gs[g];
    return o;
}

__global__ __launch_bounds__(64) void list_heap_kernel(const ListHeapArgs a)
{
    const uint32_t qi = blockIdx.x * 64u + threadIdx.x;
    if (qi >= a.q_n) return;
    const uint32_t q = a.q_lo + qi;
    const uint64_t m = a.rec_off[q + 1] - a.rec_off[q];                  // this query's records
    const uint64_t *__restrict__ rec = a.rec + (a.rec_off[q] - a.rec_off[a.q_lo]);
    const uint64_t out0 = a.res_off[q] - a.res_off[a.q_lo];
    const int64_t N = (int64_t)(m < a.nresults ? m : a.nresults);        // (a heap never grows beyond the records there are)
    if (N == 0) return;
    HeapMem h{a.key + out0 + qi, a.ref + out0 + qi};                      // N + 1 entries
    int64_t n = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const double v = hit_of(rec[i], a.sketch_size, a.genome_size, a.id_base).intersection;
        if (n >= N) {
            if (h.key[0] > v) continue;                                   // Miekki.cpp:387, ties replace
            pop_to_back(h, n);
            --n;
        }
        h.key[n] = v; h.ref[n] = (uint32_t)i;                             // push_back + push_heap
        ++n;
        sift_up(h, n - 1, 0, v, (uint32_t)i);
    }
    for (int64_t len = n; len > 1; --len) pop_to_back(h, len);            // std::sort_heap
    mk_hit *__restrict__ out = a.hits + out0;
    for (int64_t i = 0; i < n; ++i) out[i] = hit_of(rec[h.ref[i]], a.sketch_size, a.genome_size, a.id_base);
}

__global__ __launch_bounds__(256) void list_expand_kernel(const uint64_t *__restrict__ rec, uint64_t n, const uint32_t *__restrict__ ss,
                                                          const uint64_t *__restrict__ gs, uint32_t id_base, mk_hit *__restrict__ hits)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) hits[i] = hit_of(rec[i], ss, gs, id_base);
}

template <bool WRITE>
int launch_list(mk_ctx *c, const ListArgs &a)
{
    return launch_walk(c, a, "lists", nullptr, [&](auto src, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((list_kernel<decltype(src)::value, WRITE>), grid, block, 0, c->stream, a);
    });
}

}  // namespace

int launch_list_count(mk_ctx *c, const ListArgs &a) { return launch_list<false>(c, a); }
int launch_list_write(mk_ctx *c, const ListArgs &a) { return launch_list<true>(c, a); }

int launch_list_scan(mk_ctx *c, const uint32_t *d_count, uint32_t n, uint32_t nresults, uint64_t *d_rec_off, uint64_t *d_res_off)
{
    hipLaunchKernelGGL(list_scan_kernel, dim3(1), dim3(1024), 0, c->stream, d_count, n, nresults, d_rec_off, d_res_off);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_list_heap(mk_ctx *c, const ListHeapArgs &a)
{
    if (!a.q_n) return MK_OK;
    hipLaunchKernelGGL(list_heap_kernel, dim3((a.q_n + 63) / 64), dim3(64), 0, c->stream, a);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

int launch_list_expand(mk_ctx *c, const uint64_t *d_rec, uint64_t n, const uint32_t *ss, const uint64_t *gs, uint32_t id_base, mk_hit *d_hits)
{
    if (!n) return MK_OK;
    if (n > 0x7fffffffull * 256) { set_error("too many records for one launch"); return MK_ERR_ARG; }
    hipLaunchKernelGGL(list_expand_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, c->stream, d_rec, n, ss, gs, id_base, d_hits);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
