// scan_tune -- A/B timing of scan_kernel variants, interleaved rounds in ONE process
// (cdna_hip_programming.md rule 24).  Synthetic matrix (random bytes) and random
// sorted entry lists of realistic shape; timing only, plus a cross-variant checksum
// of the first score rows.  Build: make -C miekki_amd/csrc tune
//   scan_tune <G> <h> <Q> <entries_per_query> <rounds>
//   scan_tune pieces <G> <h> <rounds> [tiles] [S] [LDS KiB]   the narrow-tile gather probe (piece_probe_kernel, piece_probe32_kernel)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../miekki_amd/csrc/scan_kernel.hpp"

namespace mk { void set_error(const char *, ...) {} }
using namespace mk;

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__global__ void fill_kernel(uint4 *p, uint64_t n16, uint64_t seed)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = splitmix64(seed ^ (2 * i)), b = splitmix64(seed ^ (2 * i + 1));
        // skew towards a few values like real fingerprints: keep the high nibble in 0xC..0xF
        const uint64_t m = 0x3f3f3f3f3f3f3f3fULL, o = 0xc0c0c0c0c0c0c0c0ULL;
        const uint64_t x = (a & m) | o, y = (b & m) | o;
        p[i] = make_uint4((uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32));
    }
}


// ---- experiment: narrower row tiles (LB bytes per lane instead of 16) so that the
// tile-major column slab (2^h x 64*LB bytes) fits the Infinity Cache; store-less.
template <int LB, int UNROLL>
__global__ __launch_bounds__(256) void narrow_kernel(const ScanArgs a)
{
    constexpr uint32_t ND = LB / 4, TB = 64 * LB;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t ntiles = (a.G + TB - 1) / TB;
    const uint32_t work = blockIdx.x * 4u + wave;
    if (work >= a.nq * ntiles) return;
    const uint32_t tile = work / a.nq, ql = work - tile * a.nq;
    if ((uint64_t)tile * TB + lane * LB >= a.G) return;
    const uint64_t *__restrict__ ent = a.entries + a.ent_off[ql];
    const uint32_t n = a.nent[ql];
    const uint8_t *__restrict__ base = a.M + (uint64_t)tile * TB;
    const uint32_t voff = lane * LB;
    uint32_t tot[ND];
    for (uint32_t k = 0; k < ND; ++k) tot[k] = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 255) {
        const uint32_t m = min(n - i0, 255u);
        const uint64_t *__restrict__ e = ent + i0;
        uint32_t acc[ND];
        for (uint32_t k = 0; k < ND; ++k) acc[k] = 0;
        uint32_t j = 0;
        for (; j + UNROLL <= m; j += UNROLL) {
            uint64_t ev[UNROLL];
            uint32_t d[UNROLL][ND];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) ev[u] = e[j + u];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const uint8_t *p = row_base(base, (uint32_t)ev[u], a.ld) + voff;
                if (ND == 1) d[u][0] = *reinterpret_cast<const uint32_t *>(p);
                else if (ND == 2) { const uint2 t = *reinterpret_cast<const uint2 *>(p); d[u][0] = t.x; d[u][1] = t.y; }
                else { const uint4 t = *reinterpret_cast<const uint4 *>(p); d[u][0] = t.x; d[u][1] = t.y; d[u][2 % ND] = t.z; d[u][3 % ND] = t.w; }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const uint32_t b = bcast_fp<1>((uint32_t)(ev[u] >> 32));
#pragma unroll
                for (uint32_t k = 0; k < ND; ++k) acc[k] += ne_lanes<1>(d[u][k], b);
            }
        }
        for (; j < m; ++j) {
            const uint64_t ev = e[j];
            const uint8_t *p = row_base(base, (uint32_t)ev, a.ld) + voff;
            const uint32_t b = bcast_fp<1>((uint32_t)(ev >> 32));
            for (uint32_t k = 0; k < ND; ++k) acc[k] += ne_lanes<1>(reinterpret_cast<const uint32_t *>(p)[k], b);
        }
        for (uint32_t k = 0; k < ND; ++k) tot[k] += (acc[k] & 0xff) + ((acc[k] >> 8) & 0xff) + ((acc[k] >> 16) & 0xff) + (acc[k] >> 24);
    }
    for (uint32_t k = 0; k < ND; ++k) asm volatile("" ::"v"(tot[k]));
}

// ---- experiment (rejected)
// Phase-locked sweep: the grid holds only as many waves as the chip keeps resident
// and every wave walks the tile-major work list with the grid's stride.  All items
// cost the same (one query's sorted entry list), so the resident waves start item k
// together and sweep the partitions 0 -> 2^h side by side: the rows they touch at any
// moment lie in a narrow band of the column slab, which the Infinity Cache holds.
template <int W, int UNROLL, bool NT = false>
__global__ __launch_bounds__(256) void scan_sweep_kernel(const ScanArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t total = a.nq * a.ntiles, stride = gridDim.x * 4u;
    for (uint32_t work = blockIdx.x * 4u + wave; work < total; work += stride) {
        const uint32_t tile = work / a.nq, ql = work - tile * a.nq;
        scan_item<W, UNROLL, NT>(a, ql, tile, lane);
    }
}


// ---- experiment: the query's entry list staged in LDS (the north-star's suggestion)
// instead of SGPRs.  A workgroup = one query x four adjacent tiles (query-major), the
// list is loaded cooperatively (coalesced) into LDS once per workgroup, every wave
// then reads entry i as a broadcast ds_read_b64 and lifts it to SGPRs.
__global__ __launch_bounds__(256) void lds_kernel(const ScanArgs a)
{
    extern __shared__ uint64_t s_ent[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles4 = (a.ntiles + 3) / 4;
    const uint32_t ql = blockIdx.x / tiles4, tile = (blockIdx.x - ql * tiles4) * 4 + wave;
    const uint64_t *__restrict__ ent = a.entries + a.ent_off[ql];
    const uint32_t n = a.nent[ql];
    for (uint32_t i = threadIdx.x; i < n; i += 256) s_ent[i] = ent[i];
    __syncthreads();
    if (tile >= a.ntiles || (uint64_t)tile * kTileBytes + lane * 16u >= a.G) return;
    const uint8_t *__restrict__ base = a.M + (uint64_t)tile * kTileBytes;
    const uint32_t voff = lane * 16u;
    uint32_t tot[4] = {0, 0, 0, 0};
    for (uint32_t i0 = 0; i0 < n; i0 += 248) {
        const uint32_t m = min(n - i0, 248u);
        uint32_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0, j = 0;
        for (; j + 8 <= m; j += 8) {
            uint64_t ev[8]; uint4 d[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint64_t v = s_ent[i0 + j + u];                      // same address in every lane: broadcast
                ev[u] = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) d[u] = load_row16<false>(row_base(base, (uint32_t)ev[u], a.ld) + voff);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t b = bcast_fp<1>((uint32_t)(ev[u] >> 32));
                acc0 += ne_lanes<1>(d[u].x, b); acc1 += ne_lanes<1>(d[u].y, b);
                acc2 += ne_lanes<1>(d[u].z, b); acc3 += ne_lanes<1>(d[u].w, b);
            }
        }
        for (; j < m; ++j) {
            const uint64_t v = s_ent[i0 + j];
            const uint64_t ev = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
            const uint4 d = load_row16<false>(row_base(base, (uint32_t)ev, a.ld) + voff);
            const uint32_t b = bcast_fp<1>((uint32_t)(ev >> 32));
            acc0 += ne_lanes<1>(d.x, b); acc1 += ne_lanes<1>(d.y, b); acc2 += ne_lanes<1>(d.z, b); acc3 += ne_lanes<1>(d.w, b);
        }
        tot[0] += acc0; tot[1] += acc1; tot[2] += acc2; tot[3] += acc3;   // timing build: no widening
    }
    for (int k = 0; k < 4; ++k) asm volatile("" ::"v"(tot[k]));
}

// ---- the box's read-only stream ceiling (SURVEY.md 8d asks for it): every lane sums
// 16-byte loads over the whole matrix buffer, grid-stride, 8 loads in flight
__global__ __launch_bounds__(256) void stream_read_kernel(const uint4 *__restrict__ p, uint64_t n16, uint32_t *sink)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t acc = 0;
    for (; i + 7 * stride < n16; i += 8 * stride) {
        uint4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[i + u * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
    }
    for (; i < n16; i += stride) { const uint4 v = p[i]; acc += v.x ^ v.y ^ v.z ^ v.w; }
    if (acc == 0x12345678u) *sink = acc;                       // keeps the loads live
}

// ---- experiment: one wave owns TWO adjacent row tiles of a (query, range): the entry list is walked once per
// 2 KiB of row instead of once per 1 KiB (half the scalar work and half the waves per byte), 2 x UNROLL loads
// in flight per wave
template <int UNROLL>
__global__ __launch_bounds__(256) void scan_slab2_kernel(const SlabArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t work = blockIdx.x * 4u + wave;
    const uint32_t npairs = (a.ntiles + 1) / 2;
    if (work >= npairs * a.S * a.nq) return;
    const uint32_t tr = work / a.nq, ql = work - tr * a.nq;
    const uint32_t pair = tr / a.S, r = tr - pair * a.S;
    const uint32_t tile0 = 2 * pair, tile1 = 2 * pair + 1;
    const bool on0 = (uint64_t)tile0 * kTileBytes + lane * 16u < (uint64_t)a.G;
    const bool on1 = tile1 < a.ntiles && (uint64_t)tile1 * kTileBytes + lane * 16u < (uint64_t)a.G;
    if (!on0) return;
    const uint32_t q = a.q_begin + ql;
    const uint32_t lo = a.split[(uint64_t)q * (a.S + 1) + r], hi = a.split[(uint64_t)q * (a.S + 1) + r + 1];
    const uint64_t *__restrict__ e = a.entries + a.ent_off[q] + lo;
    const uint32_t m = hi - lo;
    const uint8_t *__restrict__ base = a.M + (uint64_t)tile0 * kTileBytes;
    const uint32_t voff = lane * 16u, voff1 = on1 ? voff + kTileBytes : voff;
    const uint64_t ld = a.ld;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t j = 0; j < m; j += UNROLL) {
        uint64_t ev[UNROLL];
        uint4 d0[UNROLL], d1[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) ev[u] = e[min(j + u, m - 1)];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint8_t *rb = row_base(base, (uint32_t)ev[u], ld);
            d0[u] = load_row16<false>(rb + voff);
            d1[u] = load_row16<false>(rb + voff1);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t keep = j + u < m ? 0xffffffffu : 0u;
            const uint32_t b = bcast_fp<1>((uint32_t)(ev[u] >> 32));
            acc[0] += ne_lanes<1>(d0[u].x, b) & keep; acc[1] += ne_lanes<1>(d0[u].y, b) & keep;
            acc[2] += ne_lanes<1>(d0[u].z, b) & keep; acc[3] += ne_lanes<1>(d0[u].w, b) & keep;
            acc[4] += ne_lanes<1>(d1[u].x, b) & keep; acc[5] += ne_lanes<1>(d1[u].y, b) & keep;
            acc[6] += ne_lanes<1>(d1[u].z, b) & keep; acc[7] += ne_lanes<1>(d1[u].w, b) & keep;
        }
    }
    uint8_t *__restrict__ out0 = a.partials + (((uint64_t)tile0 * a.S + r) * a.nq + ql) * kTileBytes + voff;
    *reinterpret_cast<uint4 *>(out0) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    if (on1) {
        uint8_t *__restrict__ out1 = a.partials + (((uint64_t)tile1 * a.S + r) * a.nq + ql) * kTileBytes + voff;
        *reinterpret_cast<uint4 *>(out1) = make_uint4(acc[4], acc[5], acc[6], acc[7]);
    }
}

// ---- the narrow-tile gather probe
// Counting a BLOCK of queries in LDS (a row piece fetched once for all the block's queries that want it) needs a tile so
// narrow that a CU's LDS holds a thousand queries' counters: T = 64 ... 256 bytes instead of 1,024.  One wave-instruction
// then covers 1024 / T different rows -- a group of T / 16 lanes each, with a per-lane (vector) row address where the
// scan kernels have a scalar one -- and the counters are added to with LDS integer adds.  Whether the fabric delivers
// such pieces at the rate of whole rows, and whether the LDS keeps up with the adds, was measured by this kernel before
// scan_block_kernel was built on it (mode `pieces`; profiles/r8_piece_probe.txt): store-less, rows drawn by a hash, the work numbered and
// dealt to the XCDs as scan_group_kernel's (xcd_workgroup), one workgroup of sixteen waves per CU, four loads in flight per wave.
__device__ __forceinline__ uint32_t probe_hash(uint32_t x)
{
    x *= 0x9E3779B1u; x ^= x >> 15; x *= 0x85EBCA77u; x ^= x >> 13; x *= 0xC2B2AE3Du; x ^= x >> 16;
    return x;
}

struct PieceProbeArgs {
    const uint8_t *M;
    uint64_t ld;
    uint32_t tile0, S, P;          // tiles from tile0 on; ranges of P / S partitions (a power of two)
    uint32_t items;                // workgroups per (tile, range): the blocks x sub-tiles of the planned kernel
    uint32_t steps;                // steps of four wave-instructions per wave
    uint32_t B;                    // ADD != 0: slots (queries of the block) whose counters the LDS holds, B x T bytes
    uint32_t pairs;                // ADD != 0: (slot, fingerprint) pairs counted per row piece
};

// T: bytes of a row per lane group (1,024: the whole wave takes one row through the scalar base, as the scan kernels).
// ADD: 0 loads only; 1 the loads and, per pair, the compare and four 32-bit LDS adds per lane, the word order rotated per lane
// group (no two lane groups of an LDS cycle on one bank); 2 the same not rotated, as scan_block_kernel adds (four lane groups
// on the same banks); 3 and 4: as 1 and 2 WITHOUT the loads (the words come from the hash): what the compare and the adds cost alone.
// A pair's slot and fingerprint are two shifts of a product, about what reading a pair costs the real kernel.
// OPT (with ADD 2), what scan_block_kernel might do otherwise (profiles/r10_piece_probe.txt): 1 a slot's counters every T + 4
// bytes (the lane groups of an LDS cycle on different banks unless their slots agree mod 4); 2 the
// fingerprint broadcast by v_perm_b32 instead of a multiply; 4 the row reached by ONE 32 x 32-bit multiply-add onto a per-lane
// base that holds everything else; 8 two 64-bit LDS adds per pair instead of four 32-bit ones.
// Round 14 (profiles/r14_piece_probe.txt), with ADD 2 and 4, and 1 and 3 for the rotation: 16 the pair comes as the READY-MADE
// word of scan_block_kernel (pair_word<1>: fingerprint << 24 | byte offset of the slot's counters) -- here one AND of the
// hash, standing for the word the kernel has from its packet: the broadcast is pair_fp's v_perm_b32 and the address one
// v_and_or_b32; 16 | 1 the same with the slots' banks spread as a pitch of T + 4 bytes spreads them (the offset any multiple
// of four bytes: the bank shift of a slot is uniform mod 32 either way; mask plus add); 32 the word index XOR-ed with
// slot & 3, pre-folded into the offset (three more address XORs per pair); 16 | 8 two 64-bit adds per ready-made pair.
// (The compare has no variant of its own: ne_lanes compiles to v_bitop3_b32, add, v_bitop3_b32, shift, and in every row.)
template <int T, int ADD, int OPT = 0>
__global__ __launch_bounds__(1024) void piece_probe_kernel(const PieceProbeArgs a)
{
    extern __shared__ uint32_t s_probe[];
    constexpr uint32_t LG = T / 16, NG = 64 / LG, NSUB = kTileBytes / T;   // lanes per row, rows per wave-instruction, sub-tiles
    constexpr bool LOAD = ADD < 3, ROT = ADD == 1 || ADD == 3;
    constexpr uint32_t SW = (OPT & 1) ? T / 4 + 1 : T / 4;   // words from slot to slot
    static_assert(OPT == 0 || ADD == 2 || (OPT >= 16 && (ADD == 4 || OPT == 16)), "the options are variants of the unrotated adds");
    static_assert(OPT < 16 || T == 128, "a ready-made offset is drawn for 1,024 slots of 128 bytes");
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    typedef __attribute__((address_space(3))) unsigned long long lds_u64;
    // the offset field of a ready-made pair word (the LDS holds 1,024 slots at either pitch: piece_probe_main checks)
    constexpr uint32_t FIELD = (OPT & 32) ? 0x1ff8cu : (OPT & 1) ? 0x1fffcu : 0x1ff80u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wg = xcd_workgroup();
    const uint32_t trl = wg / a.items, item = wg - trl * a.items;
    const uint32_t tile = a.tile0 + trl / a.S, r = trl % a.S, sub = item % NSUB;
    const uint32_t span = a.P / a.S, rlo = r * span;
    if (ADD) {
        for (uint32_t i = threadIdx.x; i < a.B * SW; i += 1024) s_probe[i] = 0;
        __syncthreads();
    }
    const uint8_t *__restrict__ base = a.M + (uint64_t)tile * kTileBytes + sub * T;
    const uint32_t grp = lane / LG, voff = (lane % LG) * 16u;
    const uint8_t *__restrict__ mine_base = base + voff + (uint64_t)rlo * a.ld;   // (OPT 4)
    const uint32_t ld32 = (uint32_t)a.ld;
    const uint32_t seed = (wg * 16u + wave) * (a.steps * 4u * NG);
    const uint32_t rot = ROT ? grp & 3u : 0u, slot_mask = a.B - 1u;    // (ADD: B is a power of two)
    const uint32_t l16 = (lane % LG) * 16u;
    uint32_t *mine[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) mine[j] = s_probe + (lane % LG) * 4u + ((j + rot) & 3u);
    uint32_t sink = 0;
#pragma unroll 1
    for (uint32_t st = 0; st < a.steps; ++st) {                          // (not unrolled: four loads in flight, no more)
        uint32_t hsh[4];
        uint4 d[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            hsh[u] = probe_hash(seed + (st * 4u + u) * NG + grp);
            const uint32_t p = rlo + (hsh[u] & (span - 1u));
            if (!LOAD) d[u] = make_uint4(hsh[u], hsh[u] * 3u, hsh[u] * 5u, hsh[u] * 7u);
            else if (T == (int)kTileBytes) d[u] = load_row16<false>(row_base(base, p, a.ld) + voff);
            else if (OPT & 4) d[u] = load_row16<false>(mine_base + (uint64_t)(hsh[u] & (span - 1u)) * ld32);
            else d[u] = load_row16<false>(base + (uint64_t)p * a.ld + voff);   // (a 64-bit pitch: two multiply-adds, as scan_block_kernel had)
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            if (!ADD) { sink ^= d[u].x ^ d[u].y ^ d[u].z ^ d[u].w; continue; }
            const uint32_t w0 = d[u].x, w1 = d[u].y, w2 = d[u].z, w3 = d[u].w;
            const uint32_t dr[4] = {rot == 0 ? w0 : rot == 1 ? w1 : rot == 2 ? w2 : w3, rot == 0 ? w1 : rot == 1 ? w2 : rot == 2 ? w3 : w0,
                                    rot == 0 ? w2 : rot == 1 ? w3 : rot == 2 ? w0 : w1, rot == 0 ? w3 : rot == 1 ? w0 : rot == 2 ? w1 : w2};
            for (uint32_t k = 0; k < a.pairs; ++k) {
                const uint32_t hk = hsh[u] * (2u * k + 3u);
                if (OPT & 48) {                                          // (s_probe is the kernel's only LDS: an offset is an address)
                    const uint32_t pw = hk & (0xff000000u | FIELD), b = pair_fp<1>(pw);
                    uint32_t at[4];
                    if (ROT) {
#pragma unroll
                        for (uint32_t j = 0; j < 4; ++j) at[j] = (pw & FIELD) + l16 + 4u * ((j + rot) & 3u);
                    } else {
                        const uint32_t a0 = (OPT & 1) ? (pw & FIELD) + l16 : (pw & FIELD) | l16;
#pragma unroll
                        for (uint32_t j = 0; j < 4; ++j) at[j] = (OPT & 32) ? a0 ^ (4u * j) : a0 + 4u * j;
                    }
                    if (OPT & 8) {
#pragma unroll
                        for (uint32_t j = 0; j < 4; j += 2)
                            __hip_atomic_fetch_add(reinterpret_cast<lds_u64 *>((uintptr_t)at[j]),
                                                   (unsigned long long)ne_lanes<1>(dr[j], b) | (unsigned long long)ne_lanes<1>(dr[j + 1], b) << 32,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        continue;
                    }
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                        __hip_atomic_fetch_add(reinterpret_cast<lds_u32 *>((uintptr_t)at[j]), ne_lanes<1>(dr[j], b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    continue;
                }
                const uint32_t so = ((hk >> 20) & slot_mask) * SW, fp = 0xC0u | ((hk >> 8) & 0x3fu);
                const uint32_t b = (OPT & 2) ? __builtin_amdgcn_perm(fp, fp, 0u) : bcast_fp<1>(fp);
                if (OPT & 8) {                                           // (a byte that overflows carries into the next word here: timing only)
#pragma unroll
                    for (uint32_t j = 0; j < 4; j += 2)
                        __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(mine[j] + so),
                                               (unsigned long long)ne_lanes<1>(dr[j], b) | (unsigned long long)ne_lanes<1>(dr[j + 1], b) << 32,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    continue;
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j)
                    __hip_atomic_fetch_add(mine[j] + so, ne_lanes<1>(dr[j], b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    if (ADD) {
        __syncthreads();
        sink = s_probe[threadIdx.x];
    }
    asm volatile("" ::"v"(sink));                                       // keeps the loads (the adds) live
}

// The same gather with 32 bytes per lane: a QUAD per 128-byte piece, sixteen pieces per wave-instruction, two pieces in flight
// per quad and two 16-byte loads per piece -- the four load instructions and 4 KiB per wave and step of the kernel above, the row
// reached by one multiply-add (its OPT 4).  SPLIT 0: lane l takes bytes [32 l, 32 l + 32) of the piece; 1: [16 l, 16 l + 16) and
// [64 + 16 l, 64 + 16 l + 16), so that a load instruction asks for half a line per quad, contiguously.  ADD 0: loads only; 2: the
// compare and the adds of `pairs` pairs per piece, unrotated; U64: two 64-bit LDS adds per 16 bytes in place of four 32-bit ones.
template <int SPLIT, int ADD, int U64>
__global__ __launch_bounds__(1024) void piece_probe32_kernel(const PieceProbeArgs a)
{
    extern __shared__ uint32_t s_probe[];
    constexpr uint32_t T = 128, LP = 4, NG = 64 / LP, NSUB = kTileBytes / T, SW = T / 4, HSTEP = SPLIT ? LP * 16u : 16u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wg = xcd_workgroup();
    const uint32_t trl = wg / a.items, item = wg - trl * a.items;
    const uint32_t tile = a.tile0 + trl / a.S, r = trl % a.S, sub = item % NSUB;
    const uint32_t span = a.P / a.S, rlo = r * span;
    if (ADD) {
        for (uint32_t i = threadIdx.x; i < a.B * SW; i += 1024) s_probe[i] = 0;
        __syncthreads();
    }
    const uint32_t grp = lane / LP, voff = (SPLIT ? lane % LP : lane % LP * 2u) * 16u;
    const uint8_t *__restrict__ mine_base = a.M + (uint64_t)tile * kTileBytes + sub * T + voff + (uint64_t)rlo * a.ld;
    const uint32_t ld32 = (uint32_t)a.ld;
    const uint32_t seed = (wg * 16u + wave) * (a.steps * 2u * NG), slot_mask = a.B - 1u;
    uint32_t *mine = s_probe + voff / 4u;
    uint32_t sink = 0;
#pragma unroll 1
    for (uint32_t st = 0; st < a.steps; ++st) {
        uint32_t hsh[2];
        uint4 d[2][2];
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            hsh[u] = probe_hash(seed + (st * 2u + u) * NG + grp);
            const uint8_t *row = mine_base + (uint64_t)(hsh[u] & (span - 1u)) * ld32;
            d[u][0] = load_row16<false>(row);
            d[u][1] = load_row16<false>(row + HSTEP);
        }
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u) {
            if (!ADD) { sink ^= d[u][0].x ^ d[u][0].y ^ d[u][0].z ^ d[u][0].w ^ d[u][1].x ^ d[u][1].y ^ d[u][1].z ^ d[u][1].w; continue; }
            for (uint32_t k = 0; k < a.pairs; ++k) {
                const uint32_t hk = hsh[u] * (2u * k + 3u);
                const uint32_t so = ((hk >> 20) & slot_mask) * SW, fp = 0xC0u | ((hk >> 8) & 0x3fu);
                const uint32_t b = bcast_fp<1>(fp);
#pragma unroll
                for (uint32_t hf = 0; hf < 2; ++hf) {
                    uint32_t *c = mine + so + hf * (HSTEP / 4u);
                    const uint32_t w[4] = {d[u][hf].x, d[u][hf].y, d[u][hf].z, d[u][hf].w};
                    if (U64) {                                               // (a byte that overflows carries into the next word here: timing only)
#pragma unroll
                        for (uint32_t j = 0; j < 4; j += 2)
                            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(c + j),
                                                   (unsigned long long)ne_lanes<1>(w[j], b) | (unsigned long long)ne_lanes<1>(w[j + 1], b) << 32,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    } else {
#pragma unroll
                        for (uint32_t j = 0; j < 4; ++j)
                            __hip_atomic_fetch_add(c + j, ne_lanes<1>(w[j], b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
    }
    if (ADD) {
        __syncthreads();
        sink = s_probe[threadIdx.x];
    }
    asm volatile("" ::"v"(sink));                                       // keeps the loads (the adds) live
}

// The probe's run: T-byte pieces of uniformly random rows of one range
// of the resident matrix, 1024 / T rows per wave-instruction, against whole 1 KiB rows -- the same bytes, the same rows'
// distribution, the same workgroups and occupancy (one of sixteen waves per CU: every variant asks for the LDS the
// counting kernel would).  Then the same with the compare and the LDS adds of `pairs` (slot, fingerprint) pairs per piece,
// every lane group busy, and the compare and the adds alone.
struct ProbeVariant { const char *name; void (*fn)(const PieceProbeArgs); uint32_t T, add, pairs; };

static int piece_probe_main(int argc, char **argv)
{
    const uint32_t G = argc > 2 ? atoi(argv[2]) : 100000;
    const uint32_t h = argc > 3 ? atoi(argv[3]) : 20;
    const int rounds = argc > 4 ? atoi(argv[4]) : 5;
    const uint32_t tiles = argc > 5 ? atoi(argv[5]) : 16;
    const uint32_t S = argc > 6 ? atoi(argv[6]) : 8;
    const uint32_t P = 1u << h;
    const uint64_t ld = ((uint64_t)G + kTileBytes - 1) / kTileBytes * kTileBytes;
    if (tiles == 0 || tiles > ld / kTileBytes || S == 0 || (S & (S - 1)) || S > P) { fprintf(stderr, "pieces: tiles 1..%u, S a power of two\n", (unsigned)(ld / kTileBytes)); return 1; }
    uint8_t *M; CK(hipMalloc((void **)&M, (uint64_t)P * ld));
    hipLaunchKernelGGL(fill_kernel, dim3(8192), dim3(256), 0, 0, (uint4 *)M, (uint64_t)P * ld / 16, 0x1234567ULL);
    CK(hipDeviceSynchronize());
    // the counters of a block: 152 KiB = 1,216 queries x 128 bytes (argv[7] = 160: 1,280 queries, all of a CU's LDS)
    const uint32_t kLds = (argc > 7 ? (uint32_t)atoi(argv[7]) : 152u) << 10;
    const ProbeVariant vars[] = {
        {"rows_1KiB", piece_probe_kernel<1024, 0>, 1024, 0, 0},
        {"pieces_256B", piece_probe_kernel<256, 0>, 256, 0, 0},
        {"pieces_128B", piece_probe_kernel<128, 0>, 128, 0, 0},
        {"pieces_64B", piece_probe_kernel<64, 0>, 64, 0, 0},
        {"128B_add_rot_x1", piece_probe_kernel<128, 1>, 128, 1, 1},
        {"128B_add_rot_x2", piece_probe_kernel<128, 1>, 128, 1, 2},
        {"128B_add_rot_x3", piece_probe_kernel<128, 1>, 128, 1, 3},
        {"128B_add_x2", piece_probe_kernel<128, 2>, 128, 2, 2},
        {"128B_add_x2_s33", piece_probe_kernel<128, 2, 1>, 128, 2, 2},
        {"128B_add_x2_perm", piece_probe_kernel<128, 2, 2>, 128, 2, 2},
        {"128B_add_x2_mad", piece_probe_kernel<128, 2, 4>, 128, 2, 2},
        {"128B_add_x2_s33permmad", piece_probe_kernel<128, 2, 7>, 128, 2, 2},
        {"128B_add_x2_u64", piece_probe_kernel<128, 2, 8>, 128, 2, 2},
        {"q32_pieces", piece_probe32_kernel<0, 0, 0>, 128, 0, 0},
        {"q32split_pieces", piece_probe32_kernel<1, 0, 0>, 128, 0, 0},
        {"q32_add_x2", piece_probe32_kernel<0, 2, 0>, 128, 2, 2},
        {"q32_add_x2_u64", piece_probe32_kernel<0, 2, 1>, 128, 2, 2},
        {"q32split_add_x2", piece_probe32_kernel<1, 2, 0>, 128, 2, 2},
        {"q32split_add_x2_u64", piece_probe32_kernel<1, 2, 1>, 128, 2, 2},
        {"128B_addonly_rot_x2", piece_probe_kernel<128, 3>, 128, 3, 2},
        {"128B_addonly_x2", piece_probe_kernel<128, 4>, 128, 4, 2},
        // round 14: the ready-made pair word, and on top of it the four remedies for the adds' bank conflicts
        {"r14_add_x2_word", piece_probe_kernel<128, 2, 16>, 128, 2, 2},
        {"r14_add_x2_a_pitch33", piece_probe_kernel<128, 2, 17>, 128, 2, 2},
        {"r14_add_x2_b_xor", piece_probe_kernel<128, 2, 32>, 128, 2, 2},
        {"r14_add_x2_c_u64", piece_probe_kernel<128, 2, 24>, 128, 2, 2},
        {"r14_add_x2_d_rot", piece_probe_kernel<128, 1, 16>, 128, 1, 2},
        {"r14_addonly_x2_word", piece_probe_kernel<128, 4, 16>, 128, 4, 2},
        {"r14_addonly_x2_a_pitch33", piece_probe_kernel<128, 4, 17>, 128, 4, 2},
        {"r14_addonly_x2_b_xor", piece_probe_kernel<128, 4, 32>, 128, 4, 2},
        {"r14_addonly_x2_c_u64", piece_probe_kernel<128, 4, 24>, 128, 4, 2},
        {"r14_addonly_x2_d_rot", piece_probe_kernel<128, 3, 16>, 128, 3, 2},
        {"256B_add_rot_x1", piece_probe_kernel<256, 1>, 256, 1, 1},
        {"256B_add_rot_x2", piece_probe_kernel<256, 1>, 256, 1, 2},
        {"64B_add_rot_x2", piece_probe_kernel<64, 1>, 64, 1, 2},
    };
    const int nv = sizeof vars / sizeof vars[0];
    // (the round-14 rows draw their offsets from 1,024 slots of up to 132 bytes)
    if (kLds < (132u << 10)) { fprintf(stderr, "pieces: at least 132 KiB of LDS\n"); return 1; }
    for (int v = 0; v < nv; ++v) CK(hipFuncSetAttribute((const void *)vars[v].fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    PieceProbeArgs a{};
    a.M = M; a.ld = ld; a.tile0 = 0; a.S = S; a.P = P;
    a.items = 144;                                                     // 18 blocks x 8 sub-tiles of a 21.4k-query chunk at T = 128
    a.steps = 160;                                                     // a block's ~84,000 distinct rows of a range over sixteen waves
    const uint32_t grid = tiles * S * a.items;                          // (items is a multiple of eight: so is the grid)
    const double bytes = (double)grid * 16 * a.steps * 4 * kTileBytes;
    std::vector<std::vector<float>> ms(nv);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int r = 0; r < rounds + 1; ++r)
        for (int v = 0; v < nv; ++v) {
            a.B = 1; a.pairs = vars[v].pairs;
            while (a.B * 2 * vars[v].T <= kLds) a.B *= 2;                   // (a power of two of slots: 1,024 at T = 128)
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(vars[v].fn, dim3(grid), dim3(1024), kLds, 0, a);
            CK(hipGetLastError());
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1));
            if (r) ms[v].push_back(t);                                   // round 0 = warm-up
        }
    printf("LDS asked for per workgroup: %u KiB\n", kLds >> 10);
    printf("piece gather probe: G=%u h=%u  M=%.1f GB  %u tiles x %u ranges of %u rows, %u workgroups of 16 waves x %u steps x 4 loads  %.1f GB per launch, store-less\n",
           G, h, P * (double)ld / 1e9, tiles, S, P / S, grid, a.steps, bytes / 1e9);
    std::sort(ms[0].begin(), ms[0].end());
    const float ref = ms[0][ms[0].size() / 2];
    printf("%-20s %5s %6s %10s %10s %8s %8s\n", "variant", "T", "pairs", "median ms", "min ms", "TB/s", "vs 1KiB");
    for (int v = 0; v < nv; ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        const float med = ms[v][ms[v].size() / 2];
        printf("%-20s %5u %6u %10.3f %10.3f %8.2f %8.3f\n", vars[v].name, vars[v].T, vars[v].pairs, med, ms[v][0], bytes / med / 1e9, ref / med);
    }
    return 0;
}

struct Variant { const char *name; void (*fn)(const ScanArgs); uint32_t blocks_per_cu; uint32_t lane_bytes; };   // blocks_per_cu > 0: sweep grid

#define V(U, O, N) {"u" #U "_o" #O "_nt" #N, scan_kernel<1, U, O, N>, 0, 16}
#define S(B) {"sweep_" #B "perCU", scan_sweep_kernel<1, 8, false>, B, 16}
#define N(LB, U) {"narrow_" #LB "B_u" #U, narrow_kernel<LB, U>, 0, LB}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "pieces")) return piece_probe_main(argc, argv);
    const uint32_t G = argc > 1 ? atoi(argv[1]) : 12500;
    const uint32_t h = argc > 2 ? atoi(argv[2]) : 20;
    const uint32_t Q = argc > 3 ? atoi(argv[3]) : 20000;
    const uint32_t NE = argc > 4 ? atoi(argv[4]) : 908;
    const int rounds = argc > 5 ? atoi(argv[5]) : 5;
    const uint32_t range_div = argc > 6 ? atoi(argv[6]) : 1;      // draw partitions from [0, P / range_div): slab experiment
    const uint32_t slabS = argc > 7 ? atoi(argv[7]) : 8;           // ranges of the slab schedule
    const uint32_t P = 1u << h;
    const uint64_t ld = ((uint64_t)G + kTileBytes - 1) / kTileBytes * kTileBytes;
    uint8_t *M; CK(hipMalloc((void **)&M, (uint64_t)P * ld));
    hipLaunchKernelGGL(fill_kernel, dim3(8192), dim3(256), 0, 0, (uint4 *)M, (uint64_t)P * ld / 16, 0x1234567ULL);
    std::vector<uint64_t> ent((size_t)Q * NE), off(Q + 1);
    std::vector<uint32_t> nent(Q, NE);
    std::mt19937_64 rng(42);
    for (uint32_t q = 0; q < Q; ++q) {
        off[q] = (uint64_t)q * NE;
        std::vector<uint32_t> ps(NE);
        for (auto &p : ps) p = (uint32_t)(rng() % (P / range_div));
        std::sort(ps.begin(), ps.end());
        for (uint32_t i = 0; i < NE; ++i) ent[(size_t)q * NE + i] = make_entry(ps[i], 0xC0u | (uint32_t)(rng() & 0x3f));
    }
    off[Q] = (uint64_t)Q * NE;
    uint64_t *d_ent, *d_off; uint32_t *d_nent, *d_scores;
    const uint32_t sld = (G + kTileBytes - 1) / kTileBytes * kTileBytes;
    CK(hipMalloc((void **)&d_ent, ent.size() * 8)); CK(hipMalloc((void **)&d_off, off.size() * 8));
    CK(hipMalloc((void **)&d_nent, Q * 4)); CK(hipMalloc((void **)&d_scores, (uint64_t)Q * sld * 4));
    CK(hipMemcpy(d_ent, ent.data(), ent.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_nent, nent.data(), Q * 4, hipMemcpyHostToDevice));
    ScanArgs a{};
    a.M = M; a.Mc = nullptr; a.P_hot = 0xffffffffu; a.ld = ld; a.G = G; a.ntiles = (uint32_t)(ld / kTileBytes); a.nq = Q; a.q_begin = 0;
    a.ntiles = (G + kTileBytes - 1) / kTileBytes;
    a.entries = d_ent; a.ent_off = d_off; a.nent = d_nent; a.scores = d_scores;
    const bool tile_major_scores = getenv("SCORES_ROWS") == nullptr;
    if (getenv("NO_STORE")) a.scores = nullptr;
    const ScoreLayout lay = tile_major_scores ? score_layout_tiles(1, Q) : score_layout_rows(1, sld, G);
    a.score_tile_stride = lay.tile_stride; a.score_q_stride = lay.q_stride; a.score_vec = lay.vec;
    const Variant vars[] = {V(8, 0, false), V(8, 1, false), {"lds_staged_o0", lds_kernel, 0, 16}, N(8, 8), N(4, 8)};
    const int nv = sizeof vars / sizeof vars[0];
    const uint64_t work = (uint64_t)Q * a.ntiles;
    const uint32_t blocks = (uint32_t)((work + 3) / 4);
    const double algo = (double)Q * NE * G + 4.0 * Q * G;
    std::vector<std::vector<float>> ms(nv);
    std::vector<uint64_t> chk(nv, 0);
    // slab schedule inputs: per query the entry index of every range boundary
    std::vector<uint32_t> split((size_t)Q * (slabS + 1));
    for (uint32_t q = 0; q < Q; ++q)
        for (uint32_t r = 0; r <= slabS; ++r) {
            const uint64_t bound = (uint64_t)r * (P / slabS);
            uint32_t i = 0;
            while (i < NE && (uint32_t)ent[(size_t)q * NE + i] < bound) ++i;
            split[(size_t)q * (slabS + 1) + r] = r == slabS ? NE : i;
        }
    uint32_t *d_split; uint8_t *d_part;
    CK(hipMalloc((void **)&d_split, split.size() * 4));
    CK(hipMemcpy(d_split, split.data(), split.size() * 4, hipMemcpyHostToDevice));
    CK(hipMalloc((void **)&d_part, (uint64_t)a.ntiles * slabS * Q * kTileBytes));
    SlabArgs sa;
    sa.chunk = 0; sa.nent = nullptr; sa.Mc = nullptr; sa.P_hot = 0xffffffffu; sa.r_begin = 0;
    sa.M = M; sa.ld = ld; sa.G = G; sa.ntiles = a.ntiles; sa.nq = Q; sa.q_begin = 0; sa.S = slabS; sa.r_count = slabS;
    sa.entries = d_ent; sa.ent_off = d_off; sa.split = d_split; sa.partials = d_part;
    std::vector<float> slab_ms;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipDeviceSynchronize());
    for (int r = 0; r < rounds + 1; ++r)
        for (int v = 0; v < nv; ++v) {
            CK(hipEventRecord(e0, 0));
            uint32_t grid = vars[v].blocks_per_cu ? std::min(blocks, 256u * vars[v].blocks_per_cu) : blocks;
            if (vars[v].lane_bytes != 16 || vars[v].fn == (void (*)(const ScanArgs))narrow_kernel<16, 8>) {
                const uint32_t tb = 64 * vars[v].lane_bytes;
                grid = (uint32_t)(((uint64_t)Q * ((G + tb - 1) / tb) + 3) / 4);
            }
            size_t lds = 0;
            if (vars[v].fn == lds_kernel) { grid = Q * ((a.ntiles + 3) / 4); lds = (size_t)NE * 8; }
            hipLaunchKernelGGL(vars[v].fn, dim3(grid), dim3(256), lds, 0, a);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1));
            if (r) ms[v].push_back(t);                     // round 0 = warm-up
            else {
                if (!a.scores) continue;
                std::vector<uint32_t> c((size_t)Q * sld);                 // checksum of all scores
                CK(hipMemcpy(c.data(), d_scores, c.size() * 4, hipMemcpyDeviceToHost));
                for (uint32_t r = 0; r < Q; ++r)
                    for (uint32_t g = 0; g < G; ++g) {
                        const uint32_t t = g / kTileBytes, w = g % kTileBytes;
                        chk[v] += c[(size_t)t * lay.tile_stride + (size_t)r * lay.q_stride + w];
                    }
            }
        }
    for (int r = 0; r < rounds + 1; ++r) {
        const uint64_t sw = (uint64_t)a.ntiles * slabS * Q;
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((scan_slab_kernel<1, 8>), dim3((uint32_t)((sw + 3) / 4)), dim3(256), 0, 0, sa);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t; CK(hipEventElapsedTime(&t, e0, e1));
        if (r) slab_ms.push_back(t);
    }
    std::vector<float> slab2_ms[2];
    for (int r = 0; r < rounds + 1; ++r)
        for (int v = 0; v < 2; ++v) {
            const uint64_t sw = (uint64_t)((a.ntiles + 1) / 2) * slabS * Q;
            CK(hipEventRecord(e0, 0));
            if (v == 0) hipLaunchKernelGGL((scan_slab2_kernel<4>), dim3((uint32_t)((sw + 3) / 4)), dim3(256), 0, 0, sa);
            else        hipLaunchKernelGGL((scan_slab2_kernel<8>), dim3((uint32_t)((sw + 3) / 4)), dim3(256), 0, 0, sa);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1));
            if (r) slab2_ms[v].push_back(t);
        }
    for (int v = 0; v < 2; ++v) {
        std::sort(slab2_ms[v].begin(), slab2_ms[v].end());
        printf("slab2_u%d       median %8.3f ms  min %8.3f ms  -> %7.1f GB/s (median)  [two tiles per wave]\n", v ? 8 : 4,
               slab2_ms[v][slab2_ms[v].size() / 2], slab2_ms[v][0], algo / slab2_ms[v][slab2_ms[v].size() / 2] / 1e6);
    }
    // check the slab partials against the plain kernel's scores for the first queries
    if (a.scores) {
        hipLaunchKernelGGL((scan_kernel<1, 8, 1, false>), dim3(blocks), dim3(256), 0, 0, a);
        std::vector<uint32_t> sc((size_t)Q * sld);
        CK(hipMemcpy(sc.data(), d_scores, sc.size() * 4, hipMemcpyDeviceToHost));
        std::vector<uint8_t> pt((size_t)a.ntiles * slabS * Q * kTileBytes);
        CK(hipMemcpy(pt.data(), d_part, pt.size(), hipMemcpyDeviceToHost));
        uint64_t bad = 0;
        for (uint32_t q = 0; q < std::min<uint32_t>(Q, 50); ++q)
            for (uint32_t g = 0; g < G; ++g) {
                const uint32_t t = g / kTileBytes, w = g % kTileBytes;
                uint32_t ne = 0;
                for (uint32_t r = 0; r < slabS; ++r) ne += pt[(((size_t)t * slabS + r) * Q + q) * kTileBytes + w];
                bad += (NE - ne) != sc[(size_t)t * lay.tile_stride + (size_t)q * lay.q_stride + w];
            }
        printf("slab vs plain mismatches (first 50 queries): %llu\n", (unsigned long long)bad);
    }
    printf("range 1/%u  scores %s  G=%u h=%u Q=%u entries=%u  M=%.1f GB  algorithmic %.1f GB per launch\n", range_div, tile_major_scores ? "tile-major" : "row-major", G, h, Q, NE, P * (double)ld / 1e9, algo / 1e9);
    for (int v = 0; v < nv; ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        const float med = ms[v][ms[v].size() / 2], mn = ms[v][0];
        printf("%-14s median %8.3f ms  min %8.3f ms  -> %7.1f GB/s (median)  %7.1f (min)  chk %llu\n", vars[v].name, med, mn,
               algo / med / 1e6, algo / mn / 1e6, (unsigned long long)chk[v]);
    }
    {   // read-only stream over the same buffer
        uint32_t *d_sink; CK(hipMalloc((void **)&d_sink, 4));
        const uint64_t n16 = (uint64_t)P * ld / 16;
        std::vector<float> t;
        for (int r = 0; r < rounds + 1; ++r) {
            CK(hipEventRecord(e0, 0));
            hipLaunchKernelGGL(stream_read_kernel, dim3(256 * 8), dim3(256), 0, 0, (const uint4 *)M, n16, d_sink);
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r) t.push_back(ms);
        }
        std::sort(t.begin(), t.end());
        printf("%-14s median %8.3f ms  min %8.3f ms  -> %7.1f GB/s (median)  [read-only stream of the %.1f GB matrix]\n", "stream_read",
               t[t.size() / 2], t[0], (double)P * ld / t[t.size() / 2] / 1e6, (double)P * ld / 1e9);
    }
    std::sort(slab_ms.begin(), slab_ms.end());
    printf("%-14s median %8.3f ms  min %8.3f ms  -> %7.1f GB/s (median)  [S=%u, partials %.1f GB]\n", "slab", slab_ms[slab_ms.size() / 2],
           slab_ms[0], algo / slab_ms[slab_ms.size() / 2] / 1e6, slabS, (double)a.ntiles * slabS * Q * kTileBytes / 1e9);
    return 0;
}
