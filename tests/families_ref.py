"""The yardstick of the family tests (tests/test_gpu_families.py, tests/test_gpu_cli_families.py): the oracle's
query_sequence of every genome's sequence, the pass test of filter_results in numpy float64 exactly as
miekki_amd.index.filter_results writes it, and a plain union-find.  Nothing here touches the code under test."""
import numpy as np

import synth


def passes(rows, ss, gs, min_score, min_intersection):
    """lists[i, j]: genome j passes Miekki.cpp:381-384 for the scores rows[i]"""
    rows = np.asarray(rows, np.uint32)
    with np.errstate(divide="ignore", invalid="ignore"):
        jac = rows.astype(np.float64) / ss
        inter = jac * gs
    return (rows >= min_score) & ~(inter < min_intersection)


def intersections(rows, ss, gs):
    with np.errstate(divide="ignore", invalid="ignore"):
        return rows.astype(np.float64) / ss * gs


def union_find_labels(n_ids, pairs):
    """label per id = the smallest id of its connected component"""
    parent = list(range(n_ids))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n_ids)], np.uint32)


def family_labels(lists, query_ids=None, n_ids=None):
    """lists[q, g] -> labels over n_ids ids; query q stands for query_ids[q] (default: genome q itself)"""
    nq, G = lists.shape
    query_ids = np.arange(nq) if query_ids is None else np.asarray(query_ids)
    n_ids = max(G, int(query_ids.max()) + 1 if nq else 0) if n_ids is None else n_ids
    qq, gg = np.nonzero(lists)
    return union_find_labels(n_ids, zip(query_ids[qq], gg))


def format_labels(labels):
    """the bytes of `miekki -F`: families by ascending label, members ascending, one blank line between families"""
    fam = {}
    for j, l in enumerate(labels):
        fam.setdefault(int(l), []).append(j)
    return b"\n".join(b"".join(b"%d\n" % j for j in fam[l]) for l in sorted(fam))


def summary_line(labels):
    sizes = np.bincount(np.asarray(labels, np.int64))
    sizes = sizes[sizes > 0]
    return b"families: %d, largest %d, singletons %d" % (len(sizes), sizes.max() if len(sizes) else 0, int((sizes == 1).sum()))


class Collection:
    """G genomes of 2-3 kb at -k 15 -h 9: unrelated ones (families of one) and, at places that straddle the 64-id sets and
    the score tiles (512 or 1,024 genomes), planted relatives:
      * two species with five and four strains (synth.strain), the second with members cut to different lengths;
      * a chain a - b - c of successive synth.mutate descendants: the ends are twice as far apart as the neighbours;
      * a genome and its own first half: what each is of the other differs (sketch_size, genome_size of the target)."""

    K, H, B, THRESHOLD = 15, 9, 32, 20

    def __init__(self, G, fp_bits, seed):
        self.G, self.fp_bits, self.par = G, fp_bits, (self.K, self.H, fp_bits, self.B, self.THRESHOLD)
        tile = 1024 * 8 // fp_bits                       # genomes per score tile
        assert G > tile + 40 and G % 8
        seqs = [synth.genome_bases(seed + g, 0, 2000 + (g * 37) % 1001) for g in range(G)]
        self.species_a = [3, 64, tile - 1, tile, G - 1]
        for t, g in enumerate(self.species_a):
            seqs[g] = synth.strain(seed + 5000, t, 3000, 0.012)
        self.species_b = [63, 65, tile // 2 + 7, tile + 20]
        for t, g in enumerate(self.species_b):
            seqs[g] = synth.strain(seed + 5001, t, 3000, 0.012)[:3000 - 250 * t]
        self.chain = [10, tile - 30, tile + 33]
        a = synth.genome_bases(seed + 5002, 0, 2600)
        b = synth.mutate(a, seed % 1000 + 1, 0.02)
        c = synth.mutate(b, seed % 1000 + 2, 0.02)
        for g, s in zip(self.chain, (a, b, c)):
            seqs[g] = s
        self.nested = [130, tile + 5]
        whole = synth.genome_bases(seed + 5003, 0, 3000)
        seqs[self.nested[0]], seqs[self.nested[1]] = whole, whole[:1500]
        self.seqs = seqs


    def threshold_between_chain_links(self, inter):
        """a min_intersection taken from the oracle's rows: halfway between the chain's ends (which must not list each other)
        and the weakest of its four neighbour links (which must hold)"""
        a, b, c = self.chain
        ends = max(inter[a, c], inter[c, a])
        links = min(inter[a, b], inter[b, a], inter[b, c], inter[c, b])
        assert ends < links
        return 0.5 * (ends + links)


class Answer:
    """genomes, their oracle, and query_sequence of every genome's sequence (once)"""

    def __init__(self, par, seqs):
        from oracle import oracle as orc
        self.par, self.seqs = par, seqs
        self.o = orc.OracleMiekki(*par)
        self.o.insert_sequences(seqs)
        memo = {}
        for s in set(seqs):
            memo[s] = self.o.query_sequence(s)[0]
        self.rows = np.stack([memo[s] for s in seqs])
        self.ss, self.gs = self.o.sketch_size, self.o.genome_size
        self.threshold = par[4]

    def lists(self, min_score, min_intersection, rows=None):
        return passes(self.rows if rows is None else rows, self.ss, self.gs, min_score, min_intersection)

    def labels(self, min_score=10, min_intersection=None):
        mi = 0.5 * self.threshold if min_intersection is None else min_intersection
        return family_labels(self.lists(min_score, mi))

    def build(self, hip, lo=0, hi=None, genome_id_base=0):
        hi = len(self.seqs) if hi is None else hi
        ix = hip.Miekki(*self.par, genome_id_base=genome_id_base)
        for i in range(lo, hi, 64):
            ix.insert_sequences(self.seqs[i:min(i + 64, hi)])
        return ix
