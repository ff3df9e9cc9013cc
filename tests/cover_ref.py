"""The yardstick of the cover tests (tests/test_gpu_cover.py, tests/test_gpu_cli_cover.py): seen[P, 2^fp_bits] from the oracle's
own gated sketch of every query (minhash_sketch_partition_solid_kmers), covered from its stored columns.  Nothing here touches
the code under test."""
import numpy as np


def empty_of(o):
    return (1 << o.number_bit_minimizer) - 1


def seen(o, queries):
    """bool [P, 2^fp_bits]: some query has the gated sketch value v != empty at partition p"""
    P, bits = o.P, o.number_bit_minimizer
    s = np.zeros((P, 1 << bits), bool)
    parts = np.arange(P)
    for q in queries:
        fp = o.minhash_sketch_partition_solid_kmers(q).astype(np.int64)
        live = fp != empty_of(o)
        s[parts[live], fp[live]] = True
    return s


def stored(o):
    """int64 [P, G]: the fingerprint of genome g at partition p (two-byte columns are big-endian in the oracle)"""
    cols = o.columns()
    if o.W == 1:
        return cols.astype(np.int64)
    return (cols[:, 0::2].astype(np.int64) << 8) | cols[:, 1::2].astype(np.int64)


def covered(o, seen_table, fps=None):
    """uint32 [G]: #{ p : column_g[p] != empty and seen(p, column_g[p]) }"""
    fps = stored(o) if fps is None else fps
    hit = seen_table[np.arange(o.P)[:, None], fps] & (fps != empty_of(o))
    return hit.sum(0).astype(np.uint32)


def pack(seen_table):
    """the device's table: bit ((p << fp_bits) + v) & 31 of uint32 word ((p << fp_bits) + v) >> 5"""
    return np.packbits(seen_table.reshape(-1), bitorder="little").view(np.uint32)


def unpack(words, P, fp_bits):
    return np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little").astype(bool).reshape(P, 1 << fp_bits)


def format_cover(cov, sketch_size):
    """the bytes of `miekki -C`: a line per genome with covered > 0, ascending id: id, covered, sketch_size"""
    return b"".join(b"%d\t%d\t%d\n" % (j, int(c), int(sketch_size[j])) for j, c in enumerate(cov) if int(c))


def summary_line(n_queries, cells, h, fp_bits, cov):
    return b"cover: %d queries, %d of %d cells seen, %d genomes covered" % (
        n_queries, int(cells), 1 << (h + fp_bits), int((np.asarray(cov) > 0).sum()))
