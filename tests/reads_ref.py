"""The yardstick of the base-quality tests (tests/test_reads_definition.py, tests/test_gpu_reads.py, tests/test_gpu_cli_reads.py):
a read with qualities is cut at its bad bases -- base j is good when qual[j] >= 33 + min_qual -- into its maximal runs of good
bases, and is ONE query whose ungated sketch is the fold of the oracle's minhash_sketch_partition over those segments, in order,
with pairs_ref's strict-< merge: per partition the smallest fingerprint, the earliest segment's on a tie, with ITS hash.  The
oracle's check_bloom (pairs_ref.gate) is then asked for that winner, and a winner it drops leaves the partition empty.  A pair
with qualities is the same fold over mate 1's segments, then mate 2's.  Score rows come from pairs_ref.rows_of.  Nothing here
touches the code under test."""
import numpy as np

import cover_ref as cv
import pairs_ref as pr

K = pr.K
MIN_QUAL = 20
GOOD, BAD = ord("I"), ord("#")              # phred 40 and phred 2


def segments(s, qual, min_qual):
    """the maximal runs of good bases of s, in order"""
    s, qual = bytes(s), bytes(qual)
    assert len(s) == len(qual)
    out, start = [], None
    for j in range(len(s)):
        if qual[j] >= 33 + min_qual:
            if start is None:
                start = j
        elif start is not None:
            out.append(s[start:j])
            start = None
    if start is not None:
        out.append(s[start:])
    return out


def ungated(o, min_qual, *reads):
    """(fp, hs) of the query made of `reads` -- one (s, qual) for a read, two for a pair"""
    empty = cv.empty_of(o)
    fp, hs = np.full(o.P, empty, np.uint16), np.zeros(o.P, np.uint64)
    for s, qual in reads:
        for seg in segments(s, qual, min_qual):
            f, h, _ = o.minhash_sketch_partition(seg)
            take = f < fp                      # strict: a tie keeps the earlier segment and ITS hash
            fp, hs = np.where(take, f, fp), np.where(take, h, hs)
    return fp, hs


def sketch(o, min_qual, *reads):
    """uint16 [P]: the gated sketch"""
    fp, hs = ungated(o, min_qual, *reads)
    empty = cv.empty_of(o)
    out = fp.copy()
    live = np.flatnonzero(fp != empty)
    out[live[~pr.gate(o, hs[live])]] = empty
    return out


def rows(o, min_qual, queries, stored=None):
    """(rows, active) of queries = [(read,) or (read 1, read 2)]"""
    return pr.rows_of(o, [sketch(o, min_qual, *q) for q in queries], stored)


def seen(o, min_qual, queries):
    """cover_ref.seen for these queries"""
    s = np.zeros((o.P, 1 << o.number_bit_minimizer), bool)
    parts = np.arange(o.P)
    for q in queries:
        fp = sketch(o, min_qual, *q).astype(np.int64)
        live = fp != cv.empty_of(o)
        s[parts[live], fp[live]] = True
    return s


def quality_counts(k, min_qual, queries):
    """(bad bases, bases, queries without a stretch of k + 1 good bases): the command line's `quality:` line"""
    bad = bases = none = 0
    for q in queries:
        left = False
        for s, qual in q:
            bases += len(s)
            bad += sum(1 for x in bytes(qual) if x < 33 + min_qual)
            left = left or any(len(seg) > k for seg in segments(s, qual, min_qual))
        none += 0 if left else 1
    return bad, bases, none


def mask(L, bad=()):
    """a quality string of L good bases with the positions `bad` below MIN_QUAL"""
    q = bytearray([GOOD]) * L
    for b in bad:
        q[b] = BAD
    return bytes(q)


def put(s, at, c):
    return s[:at] + c + s[at + len(c):]


def edge_reads(seqs):
    """[(what, s, qual)]: the masked arm's edges at MIN_QUAL, cut from a text of the sample's own genomes so that the gate
    passes k-mers and the scores are not all zero"""
    text = b"".join(seqs[:5])
    assert len(text) > 2 * 4200
    out = []
    L = 150
    s = text[300:300 + L]
    for b in (0, K - 2, K - 1, K, L - K - 1, L - K, L - 1):
        out.append(("bad base at %d of %d" % (b, L), s, mask(L, [b])))
    # two bad bases: the segment between them has d - 1 bases -- no k-mer up to k, one at k + 1, two at k + 2
    for d in (K, K + 1, K + 2, K + 3):
        out.append(("two bad bases %d apart" % d, s, mask(L, [40, 40 + d])))
        out.append(("two bad bases %d apart at the head" % d, s, mask(L, [0, d])))
    for run in ((10, 12), (60, 65), (0, 40), (100, 150), (31, 33)):
        out.append(("bad run %d:%d" % run, s, mask(L, range(*run))))
    out.append(("runs and singles", s, mask(L, list(range(33, 36)) + [70] + list(range(104, 108)))))
    out.append(("every base bad", s, mask(L, range(L))))
    out.append(("none bad", s, mask(L)))
    out.append(("threshold: a base at min_qual is good, one below is bad", s, put(put(mask(L), 50, bytes([33 + MIN_QUAL])), 90, bytes([32 + MIN_QUAL]))))
    for n in (0, K, K + 1, K + 2):
        out.append(("length %d" % n, text[500:500 + n], mask(n)))
    out.append(("length %d, its last base bad" % (K + 2), text[500:500 + K + 2], mask(K + 2, [K + 1])))
    out.append(("length %d, its first base bad" % (K + 2), text[500:500 + K + 2], mask(K + 2, [0])))
    # the steps of npad (256, 512, 4,096: 1, 2, 16 keys per thread), counted in k-mers (L - k) and in windows (L - k + 1), with
    # a segment that starts at a thread's first key (96), inside a run of two and of sixteen (101) and inside a run of sixteen
    # only (130), and a cut near the end
    for nk in (254, 255, 256, 257, 510, 511, 512, 513, 4064, 4065):
        n = nk + K
        r = text[7:7 + n]
        for bad in ((95, nk - 3), (100,), (129, 130 + K + 1)):
            out.append(("nk %d bad %s" % (nk, ",".join(map(str, bad))), r, mask(n, bad)))
    # seeds: N and lower case in a segment's seed and just past it, in the first segment (start 0) and in a later one (start 81)
    L = 220
    s = text[1000:1000 + L]
    q = mask(L, [80])
    for st in (0, 81):
        for at in (0, K - 2, K - 1):
            out.append(("N at %d of the segment at %d" % (at, st), put(s, st + at, b"N"), q))
        out.append(("lower case in the seed of the segment at %d" % st, put(s, st, s[st:st + 5].lower()), q))
        out.append(("lower case just past the seed of the segment at %d" % st, put(s, st + K - 1, s[st + K - 1:st + K + 3].lower()), q))
    out.append(("a later segment's seed invalid, the first clean", put(s, 81 + 3, b"N"), q))
    out.append(("the first segment's seed invalid, a later one clean", put(s, 3, b"N"), q))
    out.append(("both seeds invalid", put(put(s, 3, b"N"), 81 + K - 2, b"n"), q))
    out.append(("N on a bad base", put(s, 80, b"N"), q))
    out.append(("all lower case", s.lower(), q))
    # crowded buckets: the bitonic path with cuts
    rep = (b"ACGTTGCAT" * 300)[:1500]
    out.append(("repeats with cuts", rep, mask(1500, [300, 301, 900, 1499])))
    unit = text[200:260]
    out.append(("indexed repeats with cuts", (unit * 40)[:1500], mask(1500, [45, 700, 701, 702, 1400])))
    out.append(("indexed repeats, 4096 bases", (unit * 70)[:4096], mask(4096, [2000, 4000])))
    return out


def edge_pairs(seqs):
    """[(what, (a, qa), (b, qb))]: pairs with qualities at MIN_QUAL"""
    text = b"".join(seqs[:5])
    a, b = text[1200:1350], pr.revcomp(text[1500:1670])
    out = []
    cuts = ([], [0], [K - 1], [K], [70], [60, 60 + K + 2], [len(a) - 1])
    for ca in cuts:
        for cb in cuts:
            out.append(("cuts %s | %s" % (ca, cb), (a, mask(len(a), ca)), (b, mask(len(b), cb))))
    out.append(("mate 1 empty", (b"", b""), (b, mask(len(b), [70]))))
    out.append(("mate 2 empty", (a, mask(len(a), [70])), (b"", b"")))
    out.append(("both empty", (b"", b""), (b"", b"")))
    out.append(("mate 1 all bad", (a, mask(len(a), range(len(a)))), (b, mask(len(b)))))
    out.append(("mate 2's seed invalid", (a, mask(len(a))), (put(b, 2, b"N"), mask(len(b), [90]))))
    out.append(("mate 1 ends on a seed's worth", (a[:K - 1], mask(K - 1)), (b, mask(len(b)))))
    # the junction at a thread's first key, inside a run of two, of sixteen; 4,096 characters in all
    for n1 in (96, 101, 130):
        for total in (257 + K, 513 + K, 4096):
            x, y = text[7:7 + n1], pr.revcomp(text[4300:4300 + total - n1])
            out.append(("junction at %d of %d" % (n1, total), (x, mask(n1, [n1 // 2])), (y, mask(len(y), [len(y) // 2, len(y) - 2]))))
    return out


def sample_reads(seqs, n=200, seed=23):
    """n pairs with qualities cut from `seqs` (pairs_ref.sample_pairs): about one base in twenty below MIN_QUAL, the good ones
    at, just above and well above it"""
    rng = np.random.default_rng(seed)
    good = np.array([33 + MIN_QUAL, 34 + MIN_QUAL, GOOD], np.uint8)
    out = []
    for a, b in pr.sample_pairs(seqs, n, seed):
        mates = []
        for m in (a, b):
            q = good[rng.integers(0, 3, len(m))]
            bad = rng.random(len(m)) < 0.05
            q[bad] = rng.integers(33, 33 + MIN_QUAL, int(bad.sum()))
            mates.append((m, q.tobytes()))
        out.append(tuple(mates))
    return out
