// The order of the winner-takes-all pass (mk_cover_winners): genome a comes before genome b when the first of these that differs
// decides -- the larger share of its own sketch covered, covered(a) * ss(b) > covered(b) * ss(a) as an exact 64-bit product (both
// factors are below 2^32; a genome with ss = 0 has covered = 0 and compares as share 0); the larger covered; the smaller id.
// Plain C++, no GPU in it: tests/helpers/winners_check.cpp drives it as a stand-alone program.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

namespace mk {

inline bool cover_before(uint32_t cov_a, uint32_t ss_a, uint32_t a, uint32_t cov_b, uint32_t ss_b, uint32_t b)
{
    // share 0 for an empty sketch, whatever its count says: 0 / 1
    const uint64_t ca = ss_a ? cov_a : 0, cb = ss_b ? cov_b : 0, sa = ss_a ? ss_a : 1, sb = ss_b ? ss_b : 1;
    const uint64_t left = ca * sb, right = cb * sa;
    if (left != right) return left > right;
    if (cov_a != cov_b) return cov_a > cov_b;
    return a < b;
}

// order[0 .. n): the genomes best first; rank (may be null): rank[order[i]] = i
inline void cover_order(const uint32_t *covered, const uint32_t *sketch_size, uint32_t n, uint32_t *order, uint32_t *rank)
{
    std::iota(order, order + n, 0u);
    std::sort(order, order + n, [&](uint32_t a, uint32_t b) { return cover_before(covered[a], sketch_size[a], a, covered[b], sketch_size[b], b); });
    if (rank)
        for (uint32_t i = 0; i < n; ++i) rank[order[i]] = i;
}

}  // namespace mk
