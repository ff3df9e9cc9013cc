"""The yardstick of the read-pair tests (tests/test_pairs_definition.py, tests/test_gpu_pairs.py, tests/test_gpu_cli_pairs.py):
a pair (a, b) is one query whose ungated sketch is, per partition, the smaller of the two mates' fingerprints from the
oracle's minhash_sketch_partition, mate 1's on a tie (strict <) with ITS hash; the oracle's check_bloom is then asked for that
winner's hash, and a winner it drops leaves the partition empty.  Score rows and the seen table come from the oracle's stored
columns (cover_ref.stored).  tally_ref.tally, the lca_ref / clade_ref functions, o.filter_results and o.format_query_line
take the rows unchanged.  Nothing here touches the code under test."""
import numpy as np

import cover_ref as cv
import synth

K, BLOOM, THRESHOLD = 31, 33, 20
PARAMS = {8: (K, 9, 8, BLOOM, THRESHOLD), 16: (K, 10, 16, BLOOM, THRESHOLD)}     # -k 31 -h 9, 8 bits; -k 31 -h 10, 16 bits
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def gate(o, hs):
    """bool [P]: check_bloom of every hash"""
    return np.array([bool(o._L.mko_check_bloom(o._h, int(x))) for x in hs], bool)


def ungated(o, a, b):
    """(fp, hs, take_b): the pair's ungated sketch, its winners' hashes, and where mate 2 won"""
    fa, ha, _ = o.minhash_sketch_partition(a)
    fb, hb, _ = o.minhash_sketch_partition(b)
    take_b = fb < fa                      # strict: a tie keeps mate 1 and ITS hash
    fp, hs = np.where(take_b, fb, fa), np.where(take_b, hb, ha)
    return fp, hs, take_b


def sketch(o, a, b):
    """uint16 [P]: the gated sketch of the pair (a, b)"""
    fp, hs, _ = ungated(o, a, b)
    empty = cv.empty_of(o)
    out = fp.copy()
    live = np.flatnonzero(fp != empty)
    out[live[~gate(o, hs[live])]] = empty
    return out


def sketches(o, pairs):
    return [sketch(o, a, b) for a, b in pairs]


def rows_of(o, fps, stored=None):
    """(uint32 [n, G] score rows, uint32 [n] active partitions) of gated sketches `fps`, from the oracle's stored columns"""
    stored = cv.stored(o) if stored is None else stored
    empty = cv.empty_of(o)
    rows = np.zeros((len(fps), o.index_size), np.uint32)
    active = np.zeros(len(fps), np.uint32)
    for i, fp in enumerate(fps):
        live = np.flatnonzero(fp != empty)
        active[i] = len(live)
        rows[i] = (stored[live] == fp[live].astype(np.int64)[:, None]).sum(0)
    return rows, active


def rows(o, pairs, stored=None):
    return rows_of(o, sketches(o, pairs), stored)


def seen(o, pairs):
    """cover_ref.seen for pairs: bool [P, 2^fp_bits], some pair has the gated sketch value v != empty at partition p"""
    s = np.zeros((o.P, 1 << o.number_bit_minimizer), bool)
    parts = np.arange(o.P)
    for a, b in pairs:
        fp = sketch(o, a, b).astype(np.int64)
        live = fp != cv.empty_of(o)
        s[parts[live], fp[live]] = True
    return s


def genomes(n=300, first=0):
    return [synth.genome_bases(77_000 + g, 0, 2000 + (g * 37) % 1001) for g in range(first, first + n)]


def sample_pairs(seqs, n=300, seed=11):
    """n pairs cut from fragments of 200-699 bases of `seqs`: mates of 40-250 bases, a = frag[:L1], b = revcomp(frag[-L2:]),
    every second b and every third a with 3 % substitutions"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        g = int(rng.integers(0, len(seqs)))
        F = 200 + int(rng.integers(0, 500))
        off = int(rng.integers(0, len(seqs[g]) - F + 1))
        frag = seqs[g][off:off + F]
        L1, L2 = 40 + int(rng.integers(0, 211)), 40 + int(rng.integers(0, 211))
        a, b = frag[:L1], revcomp(frag[-L2:])
        if i % 2 == 1:
            b = synth.mutate(b, 2 * i + 1, 0.03)
        if i % 3 == 2:
            a = synth.mutate(a, 2 * i, 0.03)
        pairs.append((a, b))
    return pairs


class Sample:
    """300 genomes of 2,000-3,000 bases at one of PARAMS and 300 pairs cut from them; the oracle's sketches, rows and active
    counts of the pairs, once"""

    def __init__(self, bits):
        from oracle import oracle as orc
        self.par = PARAMS[bits]
        self.seqs = genomes()
        self.o = orc.OracleMiekki(*self.par)
        self.o.insert_sequences(self.seqs)
        self.pairs = sample_pairs(self.seqs)
        self.stored = cv.stored(self.o)
        self.fps = sketches(self.o, self.pairs)
        self.rows, self.active = rows_of(self.o, self.fps, self.stored)

    def build(self, hip):
        ix = hip.Miekki(*self.par)
        ix.insert_sequences(self.seqs)
        return ix
