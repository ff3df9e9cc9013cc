// The walk over a chunk's scores / partial counts that decides "passes min_score and min_intersection" (Miekki.cpp:381-384),
// once for everything that needs the decision: list.hip counts and writes records with it, family.hip joins genomes, tally.hip,
// clade.hip and lca.hip count (what those three share: walk_best.hpp), rep.hip writes bitmap rows.  Behind the device code, the
// host side of a walk's launch (launch_walk).
#pragma once
#include <type_traits>

#include "mk_internal.hpp"

namespace mk {

template <int SRC>
struct ListWalk {
    static constexpr uint32_t GPL = SRC == 0 ? 4 : 8, STEP = 64 * GPL;      // genomes per lane and per step of the wave
};

// One wave walks query q (of the chunk) over all genomes, STEP at a time, lane l holding genomes gl = g0 + l * GPL ...; after
// every step ALL lanes call sink(gl, s, pot): s[j] = matches of genome gl + j, bit j of pot = that genome passes both
// thresholds -- the latter decided in the reference's double operations behind an f32 screen.
// SRC 0: u32 scores, four genomes per lane; SRC 1 / 2: partial counts of one- / two-byte fingerprints, eight per lane.
template <int SRC, typename Sink>
__device__ __forceinline__ void list_walk(const ListArgs &a, uint32_t q, uint32_t lane, Sink &&sink)
{
    constexpr uint32_t GPL = ListWalk<SRC>::GPL, STEP = ListWalk<SRC>::STEP;
    const float screen = 0.999f * (float)a.min_inter;
    const uint32_t n_active = SRC == 0 ? 0u : a.nent[q];
    for (uint32_t g0 = 0; g0 < a.G; g0 += STEP) {
        const uint32_t gl = g0 + lane * GPL;                              // this lane's genomes
        uint32_t s[GPL], pot = 0;
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) s[j] = 0;
        if (gl < a.G) {
            const uint32_t t = gl / a.tile_genomes, wi = gl - t * a.tile_genomes;   // 256 | tile_genomes, rows padded to whole tiles
            if constexpr (SRC == 0) {
                const uint4 v = *reinterpret_cast<const uint4 *>(a.scores + ((uint64_t)t * a.nq + q) * a.tile_genomes + wi);
                s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
            } else {
                using raw_t = typename std::conditional<SRC == 1, uint2, uint4>::type;
                const uint8_t *__restrict__ p = a.partials + ((uint64_t)t * a.S * a.nq + q) * kTileBytes + (uint64_t)wi * SRC;
                const uint64_t range_stride = (uint64_t)a.nq * kTileBytes;
                uint32_t ne[GPL];
#pragma unroll
                for (uint32_t j = 0; j < GPL; ++j) ne[j] = 0;
                for (uint32_t r = 0; r < a.S; ++r) {
                    const raw_t w = *reinterpret_cast<const raw_t *>(p + (uint64_t)r * range_stride);
                    if constexpr (SRC == 1) {
                        ne[0] += w.x & 0xffu; ne[1] += (w.x >> 8) & 0xffu; ne[2] += (w.x >> 16) & 0xffu; ne[3] += w.x >> 24;
                        ne[4] += w.y & 0xffu; ne[5] += (w.y >> 8) & 0xffu; ne[6] += (w.y >> 16) & 0xffu; ne[7] += w.y >> 24;
                    } else {
                        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                        for (uint32_t d = 0; d < 4; ++d) { ne[2 * d] += ww[d] & 0xffffu; ne[2 * d + 1] += ww[d] >> 16; }
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < GPL; ++j) s[j] = n_active - ne[j];
            }
            bool any = false;
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j) any |= (gl + j < a.G) && s[j] >= a.min_score;     // Miekki.cpp:381
            if (any) {
                float rt[GPL];
                if constexpr (SRC == 0) {                                  // (the size arrays are padded to whole tiles)
                    const uint4 ss4 = *reinterpret_cast<const uint4 *>(a.sketch_size + gl);
                    const ulonglong2 gsa = *reinterpret_cast<const ulonglong2 *>(a.genome_size + gl);
                    const ulonglong2 gsb = *reinterpret_cast<const ulonglong2 *>(a.genome_size + gl + 2);
                    rt[0] = (float)gsa.x / (float)ss4.x; rt[1] = (float)gsa.y / (float)ss4.y;
                    rt[2] = (float)gsb.x / (float)ss4.z; rt[3] = (float)gsb.y / (float)ss4.w;
                } else {
                    const uint4 ra = *reinterpret_cast<const uint4 *>(a.ratio + gl), rb = *reinterpret_cast<const uint4 *>(a.ratio + gl + 4);
                    rt[0] = __uint_as_float(ra.x); rt[1] = __uint_as_float(ra.y); rt[2] = __uint_as_float(ra.z); rt[3] = __uint_as_float(ra.w);
                    rt[4] = __uint_as_float(rb.x); rt[5] = __uint_as_float(rb.y); rt[6] = __uint_as_float(rb.z); rt[7] = __uint_as_float(rb.w);
                }
#pragma unroll
                for (uint32_t j = 0; j < GPL; ++j) {
                    if (!(gl + j < a.G && s[j] >= a.min_score) || (float)s[j] * rt[j] < screen) continue;
                    const double jac = (double)s[j] / (double)a.sketch_size[gl + j];            // Miekki.cpp:382-383
                    const double inter = jac * (double)a.genome_size[gl + j];
                    if (!(inter < a.min_inter)) pot |= 1u << j;                                 // Miekki.cpp:384
                }
            }
        }
        sink(gl, s, pot);
    }
}

// ---- host side: a launch's queries lie within the chunk the scores / partials were written for
inline int walk_range(const ListArgs &a)
{
    if ((uint64_t)a.q_lo + a.q_n <= a.nq) return MK_OK;
    set_error("query range outside the chunk");
    return MK_ERR_ARG;
}

// One launch of a sink that has a kernel per SRC: the checks (`missing`: what the sink found missing among its own arguments, or
// null; `what`: its results, for the message), four queries per workgroup, and THE choice of SRC from the chunk's schedule.
// launch(std::integral_constant<int, SRC>, grid, block) launches.
template <typename Launch>
int launch_walk(mk_ctx *c, const ListArgs &a, const char *what, const char *missing, Launch launch)
{
    if (!a.q_n || !a.G) return MK_OK;
    MK_TRY(walk_range(a));
    if (missing) { set_error("%s", missing); return MK_ERR_ARG; }
    if (a.partials && (!a.ratio || !a.nent)) { set_error("%s over partial counts need the ratio array and the active counts", what); return MK_ERR_ARG; }
    const dim3 grid((a.q_n + 3) / 4), block(256);
    if (a.partials && a.W == 1) launch(std::integral_constant<int, 1>{}, grid, block);
    else if (a.partials) launch(std::integral_constant<int, 2>{}, grid, block);
    else launch(std::integral_constant<int, 0>{}, grid, block);
    MK_HIP(hipGetLastError());
    return MK_OK;
}

}  // namespace mk
