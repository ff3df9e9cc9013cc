// K6m: taxon-specific cells -- every held cell of the index credited to the deepest node of a taxonomy that contains ALL its
// holders (Kraken's k-mer LCA, from the matrix alone), and how many of a node's own cells a cover table has seen.
//
//   H'(p, v)      { g < n : leaf[g] != MK_NO_NODE, column_g[p] = v }, v != empty; n = the genomes the taxonomy was made over
//   owner(p, v)   a = min H', b = max H': climb `parent` from leaf[a] until hi > b; a climb that leaves the forest: slot n_nodes
//   specific(o)   #{ (p, v) : owner(p, v) = o }          covered(o)   #{ (p, v) : owner(p, v) = o, seen(p, v) }
//
// One read-only pass over the matrix, shaped as cover.hip's win pass.
//   walk:      per row an LDS table of two u32 per fingerprint value, both 0 for "nobody": key_lo = n - g and key_hi = g + 1,
//              each raised by an LDS atomic max -- the slot holds [a, b] = [n - key_lo, key_hi - 1].  FILTER: a plain LDS read
//              in front; a genome inside the slot's current [a, b] issues no atomic, one outside only the atomic of the side it
//              widens.  The slots only widen, so a stale read costs an atomic and never an answer.  Which genomes have a leaf
//              comes as one bit per genome (`live`, whole tiles, 0 from n on): `empty`, the padding columns and genomes
//              appended after the taxonomy was made never go in.
//   read-out:  once the row is through every non-nobody slot gives its owner (a == b: leaf[a]; else the climb over leaf,
//              parent, hi), its seen bit (one byte: the row's 32-byte slice staged in LDS; two bytes: where it lies), and is
//              cleared.  Not a second walk of the row.
//   adds:      a cell is NOT one atomic.  A wave keeps one (owner, specific, covered) triple in registers across the rows of
//              its item.  Per batch of 64 read-out lanes: the lanes whose owner is the kept one are counted into it by ballot
//              and popcount; the rest are grouped by owner, first active lane first.  A group of kStick lanes or more becomes
//              the kept triple (the old one is flushed: one relaxed agent-scope 64-bit add per non-zero counter); a smaller
//              group goes out at once, one add per counter.  An owner that collects most cells -- the root, or the slot above
//              a forest -- is the kept one nearly always and is added to a few times per wave and item; an address that is
//              added to per batch is one of many.
//   one byte:  a wave per row, 2 KiB of slots and the 32-byte slice per wave, no workgroup barrier; the next tile's load is in
//              flight.
//   two bytes: a workgroup per row, the values cut into ranges of V slots (8,192 by default: 64 KiB and the list, two
//              workgroups per CU; 16,384 is one workgroup per CU); a row passes once per range.  The lane that raises key_lo
//              from 0 appends the slot to a list of touched slots, which the read-out walks; a list that overflows (2,048
//              slots), or MIEKKI_MARK_TOUCHED=0, reads the whole range out.
#include <algorithm>
#include <cerrno>
#include <cstdlib>

#include "mk_internal.hpp"
#include "mk_device.hpp"

namespace mk {

namespace {

constexpr uint32_t kMarkTouched = 1u, kMarkNoFilter = 2u;                  // the kernels' `flags`
constexpr uint32_t kMarkList = 2048;      // touched slots a row's range may list before the whole range is read out (two bytes)
constexpr uint32_t kStick = 8;            // lanes of one owner in a batch from which that owner becomes the kept triple
constexpr uint32_t kNoNode = 0xffffffffu;

// the taxonomy and the outputs as the kernels take them
struct MarkTax {
    const uint32_t *leaf, *parent, *hi, *live;                             // live: bit g & 31 of word g >> 5, whole tiles
    uint32_t n, n_nodes;                                                   // genomes that take part (ids below n), nodes
    mk_node_markers *out;                                                  // n_nodes + 1 slots, added to
};

// the slot of value s widened to hold genome g: lo[s] = max(lo[s], n - g), hi[s] = max(hi[s], g + 1).  Returns true when this
// lane raised lo[s] from 0: it is the first holder the slot has met.
__device__ __forceinline__ bool mark_widen(uint32_t *lo, uint32_t *hi, uint32_t s, uint32_t g, uint32_t n, uint32_t flags)
{
    const uint32_t klo = n - g, khi = g + 1u;
    bool need_lo = true, need_hi = true;
    if (!(flags & kMarkNoFilter)) {
        need_lo = __hip_atomic_load(lo + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < klo;
        need_hi = __hip_atomic_load(hi + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < khi;
    }
    bool first = false;
    if (need_lo) first = __hip_atomic_fetch_max(lo + s, klo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0;
    if (need_hi) (void)__hip_atomic_fetch_max(hi + s, khi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return first;
}

// the owner of a slot that holds [a, b]; the slot above every node is n_nodes
__device__ __forceinline__ uint32_t mark_owner(const MarkTax &t, uint32_t a, uint32_t b)
{
    uint32_t v = t.leaf[a];
    if (a != b)
        while (v != kNoNode && t.hi[v] <= b) v = t.parent[v];
    return v == kNoNode ? t.n_nodes : v;
}

// a wave's kept triple (wave-uniform values)
struct MarkKept {
    uint32_t owner = kNoNode;
    uint64_t specific = 0, covered = 0;
};

__device__ __forceinline__ void mark_add(const MarkTax &t, uint32_t owner, uint64_t specific, uint64_t covered)
{
    unsigned long long *o = reinterpret_cast<unsigned long long *>(t.out + owner);
    if (specific) (void)__hip_atomic_fetch_add(o, (unsigned long long)specific, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (covered) (void)__hip_atomic_fetch_add(o + 1, (unsigned long long)covered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane of the wave writes the kept triple out (at the end of the item, or when another owner takes its place)
__device__ __forceinline__ void mark_flush(const MarkTax &t, MarkKept &k, uint32_t lane)
{
    if (k.owner != kNoNode && lane == 0) mark_add(t, k.owner, k.specific, k.covered);
    k.owner = kNoNode; k.specific = 0; k.covered = 0;
}

// A batch of read-out lanes: `active` lanes bring a cell of `owner`, seen or not.  Every lane of the wave calls this together.
__device__ __forceinline__ void mark_credit(const MarkTax &t, MarkKept &k, uint32_t lane, bool active, uint32_t owner, bool seen)
{
    uint64_t todo = __ballot(active);
    if (!todo) return;
    if (k.owner != kNoNode) {
        const uint64_t mine = __ballot(active && owner == k.owner);
        k.specific += (uint64_t)__popcll(mine);
        k.covered += (uint64_t)__popcll(__ballot(active && owner == k.owner && seen));
        todo &= ~mine;
    }
    while (todo) {                                                         // (uniform)
        const uint32_t src = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t o = (uint32_t)__shfl((int)owner, (int)src);
        const bool in = active && owner == o;
        const uint64_t grp = __ballot(in) & todo;
        const uint32_t ns = (uint32_t)__popcll(grp), nc = (uint32_t)__popcll(__ballot(in && seen) & todo);
        if (ns >= kStick || k.owner == kNoNode) {
            mark_flush(t, k, lane);
            k.owner = o; k.specific = ns; k.covered = nc;
        } else if (lane == src) {
            mark_add(t, o, ns, nc);
        }
        todo &= ~grp;
    }
}

// one slot read out and cleared: false for nobody's, else its owner
__device__ __forceinline__ bool mark_read(const MarkTax &t, uint32_t *lo, uint32_t *hi, uint32_t s, uint32_t &owner)
{
    const uint32_t klo = __hip_atomic_load(lo + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (!klo) return false;
    const uint32_t khi = __hip_atomic_load(hi + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    owner = mark_owner(t, t.n - klo, khi - 1u);
    __hip_atomic_store(lo + s, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_store(hi + s, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return true;
}

template <int W> __global__ void markers_kernel(MatRef, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t *, MarkTax);

// one byte: a wave per row, 256 slots of two words and the row's slice of `seen` of its own (values and kMarkTouched are not used)
template <>
__global__ __launch_bounds__(256) void markers_kernel<1>(MatRef M, uint64_t ld, uint32_t P, uint32_t ntiles, uint32_t rows_per_chunk, uint32_t values,
                                                         uint32_t flags, const uint32_t *__restrict__ seen, MarkTax t)
{
    __shared__ uint32_t s_lo[4][256], s_hi[4][256];
    __shared__ uint32_t s_seen[4][8];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t r_lo = blockIdx.x * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);          // (rows_per_chunk <= P <= 2^28)
    uint32_t *lo = s_lo[wave], *hi = s_hi[wave], *sl = s_seen[wave];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) { lo[lane + 64u * k] = 0; hi[lane + 64u * k] = 0; }
    MarkKept kept;
    for (uint32_t r = r_lo + wave; r < r_hi; r += 4u) {
        if (lane < 8u) sl[lane] = seen ? seen[(uint64_t)r * 8u + lane] : 0u;
        wave_sync();
        const uint8_t *row = mat_row(M, r, ld) + lane * 16u;
        uint4 cur = *reinterpret_cast<const uint4 *>(row), nxt = cur;
        for (uint32_t tl = 0; tl < ntiles; ++tl) {
            if (tl + 1 < ntiles) nxt = *reinterpret_cast<const uint4 *>(row + (uint64_t)(tl + 1) * kTileBytes);
            const uint32_t x[4] = {cur.x, cur.y, cur.z, cur.w};
            const uint32_t g0 = tl * kTileBytes + lane * 16u;
            const uint32_t alive = (t.live[g0 >> 5] >> (g0 & 31u)) & 0xffffu;                        // (0 from t.n on: padding, later genomes)
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t v = (x[j / 4] >> ((j * 8u) & 31u)) & 255u;
                if (((alive >> j) & 1u) && v != 255u) (void)mark_widen(lo, hi, v, g0 + j, t.n, flags);
            }
            cur = nxt;
        }
        wave_sync();
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t s = lane + 64u * k;
            uint32_t owner = 0;
            const bool active = mark_read(t, lo, hi, s, owner);
            mark_credit(t, kept, lane, active, owner, (sl[s >> 5] >> (s & 31u)) & 1u);
        }
        wave_sync();
    }
    mark_flush(t, kept, lane);
}

// two bytes: a workgroup per row, the values in ranges of `values` slots: s_dyn = [lo: values][hi: values][list: kMarkList][listed: 1]
template <>
__global__ __launch_bounds__(256) void markers_kernel<2>(MatRef M, uint64_t ld, uint32_t P, uint32_t ntiles, uint32_t rows_per_chunk, uint32_t values,
                                                         uint32_t flags, const uint32_t *__restrict__ seen, MarkTax t)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
    uint32_t *lo = s_dyn, *hi = s_dyn + values, *list = hi + values, *listed = list + kMarkList;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, touched = flags & kMarkTouched;
    const uint32_t r_lo = blockIdx.x * rows_per_chunk, r_hi = min(P, r_lo + rows_per_chunk);
    const uint32_t nvec = ntiles * (kTileBytes / 16u);                     // uint4s of a row: whole tiles, which ld covers
    const uint8_t *live8 = reinterpret_cast<const uint8_t *>(t.live);      // (little-endian: the byte of genomes 8 i .. 8 i + 7)
    for (uint32_t s = tid; s < 2u * values; s += 256u) s_dyn[s] = 0;
    if (tid == 0) *listed = 0;
    __syncthreads();
    MarkKept kept;
    for (uint32_t r = r_lo; r < r_hi; ++r) {
        const uint4 *row = reinterpret_cast<const uint4 *>(mat_row(M, r, ld));
        const uint32_t *sl = seen ? seen + (uint64_t)r * 2048u : nullptr;  // the row's 8 KiB slice, looked up where it lies
        for (uint32_t v0 = 0; v0 < 65536u; v0 += values) {
            uint4 cur = tid < nvec ? row[tid] : make_uint4(0, 0, 0, 0), nxt = cur;
            for (uint32_t i = tid; i < nvec; i += 256u) {
                if (i + 256u < nvec) nxt = row[i + 256u];
                const uint32_t x[4] = {cur.x, cur.y, cur.z, cur.w};
                const uint32_t alive = live8[i];                           // (0 from t.n on: padding, later genomes)
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) {
                    const uint32_t v = (x[j / 2] >> ((j * 16u) & 31u)) & 65535u;
                    if (!((alive >> j) & 1u) || v == 65535u || v - v0 >= values) continue;           // no leaf, `empty`, another range's (unsigned)
                    if (mark_widen(lo, hi, v - v0, i * 8u + j, t.n, flags) && touched) {
                        const uint32_t at = __hip_atomic_fetch_add(listed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        if (at < kMarkList) list[at] = v - v0;
                    }
                }
                cur = nxt;
            }
            __syncthreads();
            const uint32_t n = *listed;
            __syncthreads();
            if (tid == 0) *listed = 0;
            const bool by_list = touched && n <= kMarkList;
            const uint32_t end = by_list ? n : values;
            for (uint32_t i0 = tid - lane; i0 < end; i0 += 256u) {         // (uniform per wave: mark_credit is a wave's step)
                const uint32_t i = i0 + lane;
                uint32_t owner = 0, s = 0;
                bool active = i < end;
                if (active) {
                    s = by_list ? list[i] : i;
                    active = mark_read(t, lo, hi, s, owner);
                }
                const uint32_t v = v0 + s;
                mark_credit(t, kept, lane, active, owner, active && sl && ((sl[v >> 5] >> (v & 31u)) & 1u));
            }
            __syncthreads();
        }
    }
    mark_flush(t, kept, lane);
}

// a switch that is a whole number from `least` to `most`
int read_switch(const char *name, long least, long most, long *value)
{
    const char *e = getenv(name);
    if (!e) return MK_OK;
    char *end = nullptr;
    errno = 0;
    const long v = strtol(e, &end, 10);
    if (errno || end == e || *end || v < least || v > most) {
        set_error("%s takes a whole number from %ld to %ld: '%s'", name, least, most, e);
        return MK_ERR_ARG;
    }
    *value = v;
    return MK_OK;
}

// Two bytes: slots per LDS range, a power of two from 256 on; two words per slot, so 16,384 (128 KiB and the list) is the most a
// workgroup's LDS holds.
constexpr uint32_t kMarkValuesMax = 16384;
size_t markers_lds(uint32_t values) { return ((size_t)values * 2 + kMarkList + 4) * 4; }

}  // namespace

// MIEKKI_MARK_ROWS: rows per workgroup (by default about 2,048 workgroups and at least 4 rows, as the win pass);
// MIEKKI_MARK_VALUES: two bytes, the slots of a range; MIEKKI_MARK_FILTER=0 / 1: the LDS atomics without / with the plain read in
// front of them; MIEKKI_MARK_TOUCHED=0 / 1: two bytes, the whole range read out per row / the touched slots only.  The tests send
// small indexes down every path with them, tools/markers_rate.py measures them; the answer depends on none of them.
int markers_switches(const mk_ctx *c, uint32_t *rows, uint32_t *values, uint32_t *flags)
{
    long r = 0, v = c->W == 1 ? 256 : 8192, f = 1, tch = 1;
    MK_TRY(read_switch("MIEKKI_MARK_ROWS", 1, 0x7fffffffL, &r));
    MK_TRY(read_switch("MIEKKI_MARK_FILTER", 0, 1, &f));
    MK_TRY(read_switch("MIEKKI_MARK_TOUCHED", 0, 1, &tch));
    if (const char *e = getenv("MIEKKI_MARK_VALUES")) {                   // (checked at both widths, used at two bytes)
        long x = 0;
        if (read_switch("MIEKKI_MARK_VALUES", 256, kMarkValuesMax, &x) != MK_OK || (x & (x - 1))) {
            set_error("MIEKKI_MARK_VALUES takes a power of two from 256 to %u: a larger range does not fit the workgroup's LDS: '%s'", kMarkValuesMax, e);
            return MK_ERR_ARG;
        }
        if (c->W == 2) v = x;
    }
    if (rows) *rows = (uint32_t)r;
    if (values) *values = (uint32_t)v;
    if (flags) *flags = (tch ? kMarkTouched : 0u) | (f ? 0u : kMarkNoFilter);
    return MK_OK;
}

// d_out[n_nodes + 1] is ADDED to: the caller zeroes it.  d_seen may be null: nothing is covered.  d_live: a bit per genome,
// whole tiles of kTileBytes genomes, 0 from n on.  Raw cold rows.
int launch_markers(mk_ctx *c, const uint32_t *d_leaf, const uint32_t *d_parent, const uint32_t *d_hi, const uint32_t *d_live, uint32_t n,
                   uint32_t n_nodes, const uint32_t *d_seen, mk_node_markers *d_out)
{
    n = std::min(n, c->G);
    if (!n || !n_nodes) return MK_OK;
    uint32_t rows = 0, values = 0, flags = 0;
    MK_TRY(markers_switches(c, &rows, &values, &flags));
    const uint32_t ntiles = (uint32_t)(((uint64_t)n * c->W + kTileBytes - 1) / kTileBytes);           // the tiles that hold genomes below n
    if ((uint64_t)ntiles * kTileBytes > c->ld) { set_error("the matrix rows do not cover whole tiles"); return MK_ERR_STATE; }
    if (!rows) rows = (uint32_t)std::max<uint64_t>(4, ((uint64_t)c->P + 2047) / 2048);
    rows = std::min(rows, c->P);
    const dim3 grid((c->P + rows - 1) / rows), block(256);
    const MarkTax t{d_leaf, d_parent, d_hi, d_live, n, n_nodes, d_out};
    if (c->W == 1) {
        hipLaunchKernelGGL(markers_kernel<1>, grid, block, 0, c->stream, mat_ref(c), c->ld, c->P, ntiles, rows, values, flags, d_seen, t);
    } else {
        MK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(markers_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)markers_lds(kMarkValuesMax)));
        hipLaunchKernelGGL(markers_kernel<2>, grid, block, markers_lds(values), c->stream, mat_ref(c), c->ld, c->P, ntiles, rows, values, flags, d_seen, t);
    }
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
