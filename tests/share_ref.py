"""The yardstick of the abundance tests (tests/test_share_definition.py, tests/test_gpu_share.py,
tests/test_gpu_cli_abundance.py): per query the oracle's own filter_results through clade_ref.per_query -- the full list with its
intersections --, the margin rule on those intersections in Python floats (IEEE doubles) with the two products the header
writes, the pool, the rounds and the bytes of `miekki -E` in Python integers.  Nothing here touches the code under test."""
import numpy as np

import clade_ref as cr

MARGINS = (0, 10, 100)
AUTO = None
ONE = 1 << 32


def kept(listed, margin):
    """K(q): the ids of the listed genomes (clade_ref.per_query's triples) within the margin of the best one, ascending"""
    if not listed:
        return ()
    x = cr.best_of(listed)[2]
    return tuple(h[0] for h in listed if h[2] * 100.0 >= x * float(100 - margin))


class Pool:
    """queries, unique[G], shared[G] and the shared reads' lists (tuples of ascending ids), in Python integers"""

    def __init__(self, G):
        self.G, self.queries, self.unique, self.shared, self.lists = G, 0, [0] * G, [0] * G, []

    def add(self, ids):
        ids = tuple(int(g) for g in ids)
        assert all(0 <= g < self.G for g in ids) and all(a < b for a, b in zip(ids, ids[1:]))
        self.queries += 1
        if len(ids) == 1:
            self.unique[ids[0]] += 1
        elif ids:
            self.lists.append(ids)
            for g in ids:
                self.shared[g] += 1
        return self

    def add_queries(self, lists, margin):
        for listed in lists:
            self.add(kept(listed, margin))
        return self

    @property
    def settled(self):
        return sum(self.unique)

    @property
    def assigned(self):
        return self.settled + len(self.lists)

    @property
    def entries(self):
        return sum(len(l) for l in self.lists)

    def info(self):
        return {"queries": self.queries, "assigned": self.assigned, "shared_reads": len(self.lists), "entries": self.entries}

    def multiset(self):
        return sorted(self.lists)

    def offsets_ids(self):
        """(uint64 offsets [queries + 1], uint32 ids) of everything the pool was given, for mk_share_add_lists: the shared
        lists as they are, a list of one id per settled read; the unassigned queries as empty lists at the end"""
        all_lists = list(self.lists) + [(g,) for g, n in enumerate(self.unique) for _ in range(n)]
        all_lists += [()] * (self.queries - len(all_lists))
        off = np.zeros(len(all_lists) + 1, np.uint64)
        off[1:] = np.cumsum([len(l) for l in all_lists])
        return off, np.array([g for l in all_lists for g in l], np.uint32)


def pool_of(lists, margin, G):
    return Pool(G).add_queries(lists, margin)


def auto_shift(pool):
    return pool.assigned.bit_length()


def rounds(pool, R, shift=AUTO, trace=None):
    """(A_R [G] as Python integers, delta, starved reads of round R, the shift used); trace, a list, receives every round's
    (A_t, delta, starved): what fewer rounds would have returned"""
    assert R >= 1 and pool.assigned < ONE
    s = auto_shift(pool) if shift is AUTO else shift
    assert auto_shift(pool) <= s <= 32
    G = pool.G
    p = [1] * G
    before = [0] * G
    starved = 0
    for _ in range(R):
        A = [u << 32 for u in pool.unique]
        starved = 0
        for r in pool.lists:
            D = 0
            for g in r:
                D += p[g]
            if D:
                for g in r:
                    A[g] += (p[g] << 32) // D
            else:
                starved += 1
                each = ONE // len(r)
                for g in r:
                    A[g] += each
        assert sum(A) <= pool.assigned << 32 and sum(A) >= (pool.assigned << 32) - pool.entries
        delta = sum(abs(x - y) for x, y in zip(A, before))
        before = A
        p = [a >> s for a in A]
        assert all(w < ONE for w in p)
        if trace is not None:
            trace.append((A, delta, starved))
    return before, delta, starved, s


def reads_text(a):
    """a count of reads with 32 fractional bits as <whole>.<three digits>, the digits cut"""
    return b"%d.%03d" % (a >> 32, ((a & 0xffffffff) * 1000) >> 32)


def format_abundance(A, unique, shared):
    """the bytes of `miekki -E`: a line per genome with unique + shared > 0, ascending id: id, reads, unique, shared"""
    return b"".join(b"%d\t%s\t%d\t%d\n" % (g, reads_text(int(A[g])), int(unique[g]), int(shared[g]))
                    for g in range(len(A)) if int(unique[g]) + int(shared[g]))


def summary_line(pool, R, margin, delta):
    listed = sum(1 for u, s in zip(pool.unique, pool.shared) if u + s)
    return b"abundance: %d queries, %d assigned, %d shared by several genomes, %d ids stored, %d genomes listed, %d rounds, margin %d, last change %s" % (
        pool.queries, pool.assigned, len(pool.lists), pool.entries, listed, R, margin, reads_text(delta))
