"""The yardstick of the winners tests (tests/test_winners_definition.py, tests/test_gpu_winners.py, tests/test_gpu_cli_winners.py):
the order, won and claimed of the winner-takes-all screen from the oracle's gated sketches and stored columns, on top of
cover_ref's seen, stored and covered.  The order compares Fractions of Python integers.  Nothing here touches the code under
test."""
from fractions import Fraction

import numpy as np

import cover_ref as cr
import tally_ref as tr


def order(cov, ss):
    """ids best first: the larger covered / sketch_size (0 for an empty sketch), then the larger covered, then the smaller id"""
    def key(g):
        c, s = int(cov[g]), int(ss[g])
        return (-(Fraction(c, s) if s else Fraction(0)), -c, g)
    return np.array(sorted(range(len(cov)), key=key), np.int64)


def rank_of(order_ids):
    rank = np.empty(len(order_ids), np.int64)
    rank[np.asarray(order_ids, np.int64)] = np.arange(len(order_ids))
    return rank


def holders(o, seen_table, fps):
    """(cell, genome) of every stored fingerprint != empty that lies on a seen cell; cell = (p << fp_bits) + v"""
    hit = seen_table[np.arange(o.P)[:, None], fps] & (fps != cr.empty_of(o))
    p, g = np.nonzero(hit)
    return (p.astype(np.int64) << o.number_bit_minimizer) + fps[p, g], g.astype(np.int64)


def sorted_holders(o, seen_table, fps, order_ids):
    """the holders cell by cell, best rank first: (cell, genome, first-of-its-cell mask)"""
    cell, g = holders(o, seen_table, fps)
    rank = rank_of(order_ids)
    at = np.lexsort((rank[g], cell))
    cell, g = cell[at], g[at]
    first = np.ones(len(cell), bool)
    first[1:] = cell[1:] != cell[:-1]
    return cell, g, first


def won(o, seen_table, fps, order_ids):
    """(uint32 [G], claimed): the cells each genome wins, and the seen cells that some genome holds"""
    cell, g, first = sorted_holders(o, seen_table, fps, order_ids)
    return np.bincount(g[first], minlength=o.index_size).astype(np.uint32), int(first.sum())


def contested(o, seen_table, fps, cov, order_ids):
    """(cells with several holders, those of them whose two best holders have the same share of their sketches covered)"""
    cell, g, first = sorted_holders(o, seen_table, fps, order_ids)
    second = np.zeros(len(cell), bool)
    second[1:] = first[:-1] & ~first[1:]
    a, b = g[np.nonzero(second)[0] - 1], g[second]
    ss = o.sketch_size
    ties = sum(1 for x, y in zip(a.tolist(), b.tolist()) if int(cov[x]) * int(ss[y]) == int(cov[y]) * int(ss[x]))
    return int(second.sum()), ties


def format_winners(w, cov, sketch_size):
    """the bytes of `miekki -W`: a line per genome with won > 0, ascending id: id, won, covered, sketch_size"""
    return b"".join(b"%d\t%d\t%d\t%d\n" % (j, int(x), int(cov[j]), int(sketch_size[j])) for j, x in enumerate(w) if int(x))


def summary_line(n_queries, claimed, cells, w):
    return b"winners: %d queries, %d of %d seen cells held, %d genomes win cells" % (
        n_queries, int(claimed), int(cells), int((np.asarray(w) > 0).sum()))


class Sample:
    """a tr.Sample with the oracle's table, counts, order and winners of all its queries, each computed once"""

    def __init__(self, *args, **kw):
        self.s = s = tr.Sample(*args, **kw)
        self.o = o = s.o
        self.bits, self.P, self.G = o.number_bit_minimizer, o.P, o.index_size
        self.fps = stored = cr.stored(o)
        self.seen = cr.seen(o, s.queries)
        self.words = cr.pack(self.seen)
        self.cov = cr.covered(o, self.seen, stored)
        self.cells = int(self.seen.sum())
        self.nbytes = (self.P << self.bits) >> 3
        self.order = order(self.cov, o.sketch_size)
        self.won, self.claimed = won(o, self.seen, stored, self.order)

    def of(self, queries):
        """(seen, covered, order, won, claimed) of other queries against the same index"""
        seen_table = cr.seen(self.o, queries)
        cov = cr.covered(self.o, seen_table, self.fps)
        ids = order(cov, self.o.sketch_size)
        return (seen_table, cov, ids) + won(self.o, seen_table, self.fps, ids)


def samples():
    """the two samples of the winners tests, made on demand: get(8), get(16)"""
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Sample() if bits == 8 else Sample(603, 16, 320_000, whole=())
        return made[bits]
    return get
