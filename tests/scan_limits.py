"""Inputs built to sit on the packed counters' limits (not a test module itself): steered queries and the collections
around them, shared by test_scan_limit_inputs.py (the oracle alone proves the inputs) and test_gpu_scan_limits.py.

A query cut from a random genome spreads its entries evenly over the partitions, so a (query, range) of the slab
schedule holds about the mean and never exactly 255 or 256 entries.  Here a sequence is GROWN one base at a time: the
oracle says which partition each of the four possible next k-mers falls into, and the base is taken whose partition is
new in the wanted partition range -- until that range holds exactly the wanted number of partitions.  The hash is never
restated: every partition comes from OracleMiekki.minhash_sketch_partition.

A steered sequence is itself a genome of its collection: every entry of the query then passes the Bloom gate and that
genome matches all of them (a packed mismatch counter of 0x00), while its neighbours in the counter word are short
unrelated genomes chosen (with the oracle) to match none (0xff at 255 entries): where a carry or a wrong lane shows."""
import functools
import os
import sys

import numpy as np

import synth

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

_ACGT = np.frombuffer(b"ACGT", np.uint8)
BLOOM_LOG2, THRESHOLD = 32, 20
HOST_MEAN = 178            # the host doubles S by itself once the longest short query has more than S x 178 k-mers (one byte)


def kmer_partition(o, kmer):
    """Partition the k-mer falls into, None when its fingerprint equals `empty` (never stored).  One more character is
    appended because the reference skips a sequence's last k-mer."""
    fp, _, act = o.minhash_sketch_partition(bytes(kmer) + b"A")
    return int(fp.argmin()) if act else None


def range_bounds(P, S, r):
    return r * (P // S), (r + 1) * (P // S) if r + 1 < S else P


def steered(o, S, r, want, seed):
    """A sequence whose sketch has exactly `want` partitions in partition range r of S."""
    k, P = o.kmer_size, o.P
    lo, hi = range_bounds(P, S, r)
    rng = np.random.default_rng(seed)
    seq = bytearray(_ACGT[rng.integers(0, 4, k - 1)].tobytes())
    have = set()
    for _ in range(200 * want):
        cand = [int(c) for c in rng.permutation(4)]
        parts = [kmer_partition(o, seq[len(seq) - (k - 1):] + _ACGT[c:c + 1].tobytes()) for c in cand]
        good = [i for i, p in enumerate(parts) if p is not None and lo <= p < hi and p not in have]
        i = good[0] if good else 0            # (no good base: none of the four adds a partition to the range either)
        seq.append(int(_ACGT[cand[i]]))
        if good:
            have.add(parts[i])
            if len(have) == want:
                return bytes(seq) + b"A"      # one more character, so that the last k-mer counts
    raise AssertionError(f"steered({S}, {r}, {want}, {seed}): target not reached")


def all_distinct(o, n, seed):
    """A sequence of n sketched k-mers, each in a partition of its own: n k-mers, n entries.  (Where all four next
    k-mers fall into partitions already taken the walk starts again from the next seed: still deterministic.)"""
    k = o.kmer_size
    for attempt in range(16):
        rng = np.random.default_rng(seed + 1000 * attempt)
        seq = bytearray(_ACGT[rng.integers(0, 4, k - 1)].tobytes())
        have = set()
        while len(have) < n:
            for c in rng.permutation(4):
                p = kmer_partition(o, seq[len(seq) - (k - 1):] + _ACGT[c:c + 1].tobytes())
                if p is not None and p not in have:
                    have.add(p)
                    seq.append(int(_ACGT[c]))
                    break
            else:
                break
        if len(have) == n:
            return bytes(seq) + b"A"
    raise AssertionError(f"all_distinct({n}, {seed}): no walk reached the target")


def gated_partitions(o, seq):
    """Partitions of the query's entry list: the sketch's partitions whose hash passes the collection's Bloom gate."""
    fp, hs, _ = o.minhash_sketch_partition(seq)
    empty = 255 if o.W == 1 else 65535
    return np.array([p for p in np.flatnonzero(fp != empty) if o._L.mko_check_bloom(o._h, int(hs[p]))], np.int64)


def per_range(o, S, seq):
    parts = gated_partitions(o, seq)
    return np.bincount(np.minimum(parts // (o.P // S), S - 1), minlength=S)


def prefix_with_entries(o, genome, want):
    """The shortest-found prefix of an indexed genome with exactly `want` entries: a prefix one base longer changes one
    partition, i.e. the count by at most one, so the count that first reaches `want` equals it."""
    f = lambda n: len(gated_partitions(o, genome[:n]))
    lo, hi = o.kmer_size, len(genome)
    assert f(hi) >= want, "genome too short for that many entries"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(mid) >= want:
            hi = mid
        else:
            lo = mid
    assert f(hi) == want
    return genome[:hi]


class Special:
    """A built sequence that is a genome of the collection, at the ids `ids` (each of the four byte positions of a word)."""
    def __init__(self, tag, seq, r=None, want=None):
        self.tag, self.seq, self.r, self.want, self.ids = tag, seq, r, want, []


class Collection:
    pass


# (k, h, fingerprint bits, S at MIEKKI_SLAB_MIB=1, genomes -- the last 1 KiB tile ragged --, filler length, steered plan (want, range))
SHAPES = {
    "h12": (21, 12, 8, 4, 1030, 1500, [(255, 0), (255, 1), (255, 2), (255, 3), (256, 2)]),
    "h14": (21, 14, 8, 16, 1030, 3000, [(255, 0), (255, 5), (255, 15), (256, 15)]),
    "w16": (31, 14, 16, 16, 530, 3000, [(255, 0), (255, 7), (255, 15)]),
    "many": (21, 12, 8, 4, 13 * 1024 + 6, 1200, []),       # 14 tiles: 300 queries are 4,200 >= 4,096 (query, tile) waves
}


@functools.lru_cache(maxsize=None)
def collection(name):
    k, h, fpb, S, G, flen, plan = SHAPES[name]
    c = Collection()
    c.name, c.k, c.h, c.fpb, c.S, c.G, c.W = name, k, h, fpb, S, G, fpb // 8
    bare = orc.OracleMiekki(k, h, fpb, BLOOM_LOG2, THRESHOLD)          # empty: asked for partitions only
    sp = [Special(f"{want}@{r}", steered(bare, S, r, want, 1000 * want + r), r, want) for want, r in plan]
    if name == "h14":
        sp.append(Special("distinct2041", all_distinct(bare, 2041, 7)))
    if name == "many":
        sp.append(Special("distinct256", all_distinct(bare, 256, 9)))
    c.special = sp
    # one longer genome: case d's queries (h12) and case c's longest short query (h14) are its prefixes
    c.long_genome = {"h12": synth.genome_bases(77_000, 0, 8000), "h14": synth.genome_bases(88_000, 0, 6000)}.get(name)
    singles = [c.long_genome] if c.long_genome else []
    # copies: special j at ids = 0, 1, 2, 3 mod 4 in words of their own inside the first tile; the first one once more as the
    # collection's last genome, in the ragged tile
    words = min(G, 1024 // c.W) // 4 - 10
    stride = words // (4 * len(sp))
    assert stride >= 2
    place = {}
    for j, s in enumerate(sp):
        for pos in range(4):
            place[4 * (10 + stride * (4 * j + pos)) + pos] = j
    place[G - 1] = 0
    npool = G - len(place) - len(singles)
    # (the first fillers are very short: a few dozen partitions, so that enough of them match nothing -- the neighbours)
    nshort = 16 * (len(sp) + 1)
    pool = [synth.genome_bases(50_000 + i, 0, k + 40 + i % 30 if i < nshort else flen + 3 * (i % 50)) for i in range(npool)]
    # which fillers match NOTHING of a special's query: the score of a genome depends on its column and on the gate, and the
    # gate (a byte of the filter is zero or not) on the set of genomes, not on their order -- so ask an oracle over the
    # same genomes in any order
    pre = orc.OracleMiekki(k, h, fpb, BLOOM_LOG2, THRESHOLD)
    pre.insert_sequences([s.seq for s in sp] + singles + pool)
    rows = pre.query_sequences([s.seq for s in sp])[:, len(sp) + len(singles):]
    order, used = [None] * G, set()
    for g, j in sorted(place.items()):
        order[g] = sp[j].seq
        sp[j].ids.append(g)
    for g, j in sorted(place.items()):
        for n in range(g & ~3, min((g & ~3) + 4, G)):
            if order[n] is None:
                f = next(int(i) for i in np.flatnonzero(rows[j] == 0) if int(i) not in used)
                used.add(f)
                order[n] = pool[f]
    rest = iter([x for i, x in enumerate(pool) if i not in used] + singles[::-1])
    for g in range(G):
        if order[g] is None:
            order[g] = next(rest)
    c.genomes = order
    c.fillers = pool[nshort:]
    o = orc.OracleMiekki(k, h, fpb, BLOOM_LOG2, THRESHOLD)
    o.insert_sequences(order)
    c.oracle = o
    for s in sp:
        s.active = o.query_sequence(s.seq)[1]
    return c


def cut(c, i, n):
    f = c.fillers[(37 * i) % len(c.fillers)]
    return f[50 + i % 40:50 + i % 40 + n]


def set_a(c):
    """Case a: 35 queries -- two full groups of sixteen and a ragged one -- with the 255-in-one-range queries of the first
    and a middle range as neighbours in the first group, the last range's as the last query of the set, the others (if
    any) in the second group, between ordinary cut queries, an empty one and one shorter than k."""
    qs = [cut(c, i, 300 + (53 * i) % 300) for i in range(35)]
    at255 = [s for s in c.special if s.want == 255]
    where = {3: at255[0], 4: at255[1], 34: at255[-1]}
    for n, s in enumerate(at255[2:-1]):
        where[17 + 5 * n] = s
    for at, s in where.items():
        qs[at] = s.seq
    qs[20], qs[21] = b"", b"ACGTACGT"
    return qs, where


def set_b(c):
    """Case b: set a with the 256-in-one-range query added (inside the first group)."""
    qs, where = set_a(c)
    s256 = next(s for s in c.special if s.want == 256)
    qs = qs[:10] + [s256.seq] + qs[10:]
    return qs, {**{(at if at < 10 else at + 1): s for at, s in where.items()}, 10: s256}


def set_c_count(c, nk):
    """Case c (i) / (ii): 300 queries, the longest with exactly nk k-mers and nk entries (a prefix of the all-distinct
    genome), in the middle of ordinary cut queries of at most 230 k-mers."""
    s = next(s for s in c.special if s.tag.startswith("distinct"))
    qs = [cut(c, i, 120 + (29 * i) % 130) for i in range(300)]
    qs[151] = s.seq[:c.k + nk]
    return qs, 151


def set_c_long(c, nk):
    """Case c (iii): a handful of queries, the longest with nk k-mers: all in partitions of their own up to 2,041 (a prefix
    of the all-distinct genome), a prefix of the long genome beyond."""
    s = next(s for s in c.special if s.tag.startswith("distinct"))
    longest = s.seq[:c.k + nk] if nk <= 2041 else c.long_genome[:c.k + nk]
    return [cut(c, 1, 400), longest, cut(c, 2, 700), c.special[0].seq, cut(c, 3, 90)], 1


D_ENTRIES = (255, 256, 510, 511, 765)      # case d: 255 and its multiples, and one past them


def set_d(c):
    return [prefix_with_entries(c.oracle, c.long_genome, n) for n in D_ENTRIES]
