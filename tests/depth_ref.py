"""The yardstick of the depth tests (tests/test_depth_definition.py, tests/test_gpu_depth.py, tests/test_gpu_cli_depth.py):
mult[P, 2^fp_bits] from the oracle's own gated sketch of every query (minhash_sketch_partition_solid_kmers), the per-genome
median from a sort of the bytes its stored column holds.  Nothing here touches the code under test."""
import numpy as np

import cover_ref as cr

DEPTH_MAX = 255


def mult(o, queries):
    """int64 [P, 2^fp_bits], no cap: how many of the queries (a multiset) have the gated sketch value v != empty at partition p"""
    P, bits = o.P, o.number_bit_minimizer
    m = np.zeros((P, 1 << bits), np.int64)
    parts = np.arange(P)
    for q in queries:
        fp = o.minhash_sketch_partition_solid_kmers(q).astype(np.int64)
        live = fp != cr.empty_of(o)
        m[parts[live], fp[live]] += 1                    # (a partition holds one value per query: no index twice)
    return m


def table(m):
    """the device's table: uint8 [P << fp_bits], byte (p << fp_bits) + v = min(255, mult)"""
    return np.minimum(m, DEPTH_MAX).astype(np.uint8).reshape(-1)


def values(o, tab, fps=None):
    """int64 [P, G]: the table's byte at (p, column_g[p]), 0 where column_g[p] is empty"""
    fps = cr.stored(o) if fps is None else fps
    t = np.asarray(tab, np.uint8).reshape(o.P, -1)
    return np.where(fps != cr.empty_of(o), t[np.arange(o.P)[:, None], fps].astype(np.int64), 0)


def profile(o, tab, fps=None):
    """(median uint32 [G], sum uint64 [G], covered uint32 [G]) of a table: the median is the element of index
    (covered - 1) // 2 of the genome's non-zero values sorted ascending, 0 where there are none"""
    v = values(o, tab, fps)
    G = v.shape[1]
    cov = (v > 0).sum(0)
    med = np.zeros(G, np.uint32)
    for g in range(G):
        if cov[g]:
            x = np.sort(v[:, g][v[:, g] > 0])
            med[g] = x[(cov[g] - 1) // 2]
    return med, v.sum(0).astype(np.uint64), cov.astype(np.uint32)


def median_by_threshold(o, tab, fps=None):
    """the other wording: the largest t in 1..255 with #{ values >= t } >= covered // 2 + 1; 0 where covered is 0"""
    v = values(o, tab, fps)
    cov = (v > 0).sum(0)
    med = np.zeros(v.shape[1], np.uint32)
    for t in range(1, DEPTH_MAX + 1):
        med[((v >= t).sum(0) >= cov // 2 + 1) & (cov > 0)] = t
    return med


def format_depth(med, total, cov, sketch_size):
    """the bytes of `miekki -D`: a line per genome with covered > 0, ascending id: id, median, sum, covered, sketch_size"""
    return b"".join(b"%d\t%d\t%d\t%d\t%d\n" % (j, int(med[j]), int(total[j]), int(c), int(sketch_size[j])) for j, c in enumerate(cov) if int(c))


def summary_line(n_queries, cells, saturated, h, fp_bits, cov):
    return b"depth: %d queries, %d of %d cells seen, %d at 255, %d genomes covered" % (
        n_queries, int(cells), 1 << (h + fp_bits), int(saturated), int((np.asarray(cov) > 0).sum()))
