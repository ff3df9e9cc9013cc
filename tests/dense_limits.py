"""Inputs that put the dense scans' counters AT their limits, and the yardstick they are measured with: plain numpy, no GPU,
no oracle.  A matrix M[P][G] of fingerprints is what mk_index_import_columns takes, a block Q[P][n] of columns is what
mk_qset_from_columns takes as n whole-genome queries, and the score is one line of exact integer arithmetic (count).

A STEERED column belongs to one query: it equals the query's column in chosen rows and holds a near miss in every other
row, so its score is known before anything runs.  Near misses: at one byte the query's value with exactly one of its eight
bits flipped, cycling through the bits (each of the table kernel's 3 / 3 / 2-bit fields is the only differing one in
turn); at two bytes, in turn, low byte equal and high byte different, high equal and low different, the two bytes swapped.
Every other column is random: it matches every query here and there, and the yardstick counts that too.

test_dense_limit_inputs.py proves the builders' claims (every `Steer` of `meta`) by the yardstick alone;
test_gpu_dense_limits.py compares the device with the yardstick, all n x G numbers, by equality."""
import functools
from collections import namedtuple

import numpy as np

CHUNK = 16368                                  # dense_chunk_rows (mk_internal.hpp): rows a wave counts before it adds to the scores
COUNTS = (0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 4095, 4096, 4097, 8191, 8192, 16367, 16368)   # within chunk 0
OTHERS = (255, 256, 4096)                      # what every other query gets, rotating through the placements
PLACEMENTS = ("first", "last", "random")

# q: the query; col: the steered column; rows: where it equals the query (int64, sorted); counts: its score per chunk of
# CHUNK rows, as the builder MEANS it (the input test holds count() against it); tag: what it is there for
Steer = namedtuple("Steer", "q col rows counts tag")
# zero: the query that is 0 in every row (or None); gaps: queries with `empty` in some rows; lo_ff / hi_ff: two bytes only
Meta = namedtuple("Meta", "bits empty P G n tile steer zero gaps lo_ff hi_ff")


def geometry(bits):
    """(G, genomes per row tile): two row tiles of 1 KiB, the second ragged"""
    return (1030, 1024) if bits == 8 else (520, 512)


def nchunks(P):
    return -(-P // CHUNK)


def to_dump(fps, bits):
    """[P][n] fingerprints -> the bytes of dump_disk's column block: one byte as is, two bytes big-endian"""
    fps = np.asarray(fps)
    out = fps.astype(np.uint8) if bits == 8 else fps.astype(">u2").view(np.uint8)
    return np.ascontiguousarray(out).reshape(-1)


def count(Q, M, empty):
    """score[q][g] = #{p : Q[p][q] != empty and Q[p][q] == M[p][g]}, active[q] = #{p : Q[p][q] != empty}: returns
    (scores[n][G] int64, active[n] int64, per_chunk[chunks][n][G] int64 -- the same sums over rows [c CHUNK, (c + 1) CHUNK))."""
    Q, M = np.asarray(Q), np.asarray(M)
    assert Q.ndim == 2 and M.ndim == 2 and Q.shape[0] == M.shape[0]
    P, n = Q.shape
    dt = np.uint8 if empty == 0xff else np.uint16
    assert Q.min() >= 0 and M.min() >= 0 and Q.max() <= empty and M.max() <= empty
    Mt, Qt = np.ascontiguousarray(M.astype(dt)), Q.astype(dt)
    per = np.zeros((nchunks(P), n, M.shape[1]), np.int64)
    for q in range(n):                                             # (per query: one broadcast of everything is gigabytes)
        col = Qt[:, q]
        eq = (Mt == col[:, None]) & (col != empty)[:, None]
        for c in range(per.shape[0]):
            per[c, q] = eq[c * CHUNK:(c + 1) * CHUNK].sum(0, dtype=np.int64)
    return per.sum(0), (Q != empty).sum(0).astype(np.int64), per


def near_miss(col, rows, bits):
    """what a steered column holds where it must NOT match: never the query's value, nearly it"""
    col, rows = col.astype(np.int64), np.asarray(rows, np.int64)
    if bits == 8:
        return col ^ (1 << (rows % 8))
    hi, lo, bit = col >> 8, col & 0xff, 1 << ((rows // 3) % 8)
    swapped = (lo << 8) | hi
    kind = np.where((rows % 3 == 2) & (swapped == col), 0, rows % 3)   # (a value of two equal bytes is its own swap)
    return np.where(kind == 0, col ^ (bit << 8), np.where(kind == 1, col ^ bit, swapped))


def per_chunk(rows, P):
    return tuple(int(x) for x in np.bincount(np.asarray(rows, np.int64) // CHUNK, minlength=nchunks(P)))


class _Build:
    """a random matrix and random queries; steer() turns a column into a query's steered column"""

    def __init__(self, P, bits, n, seed):
        self.P, self.bits, self.n, self.empty = P, bits, n, (1 << bits) - 1
        self.G, self.tile = geometry(bits)
        self.rng = np.random.default_rng(seed)
        self.Q = self.rng.integers(0, self.empty, (P, n), dtype=np.int64)       # (never `empty`)
        self.M = self.rng.integers(0, self.empty + 1, (P, self.G), dtype=np.int64)
        self.steers, self.taken = [], set()
        self.zero, self.gaps, self.lo_ff, self.hi_ff = None, [], None, None
        self.all_rows = np.arange(P, dtype=np.int64)

    def steer(self, q, col, rows, counts, tag):
        assert 0 <= col < self.G and col not in self.taken, (col, tag)
        self.taken.add(col)
        rows = np.unique(np.asarray(rows, np.int64))
        v = near_miss(self.Q[:, q], self.all_rows, self.bits)
        v[rows] = self.Q[rows, q]
        self.M[:, col] = v
        self.steers.append(Steer(q, col, rows, tuple(counts), tag))

    def free_columns(self):
        left = np.array([g for g in range(self.G) if g not in self.taken], np.int64)
        return [int(g) for g in self.rng.permutation(left)]

    def done(self):
        meta = Meta(self.bits, self.empty, self.P, self.G, self.n, self.tile, tuple(self.steers), self.zero, tuple(self.gaps),
                    self.lo_ff, self.hi_ff)
        self.Q.setflags(write=False)
        self.M.setflags(write=False)
        return self.Q, self.M, meta


def _placed(b, q, c, how, lo=0, hi=None):
    """c rows of [lo, hi) in which query q is not empty: the first, the last, or drawn at random"""
    hi = min(b.P, CHUNK) if hi is None else hi
    avail = lo + np.flatnonzero(b.Q[lo:hi, q] != b.empty)
    assert c <= len(avail), (q, c, len(avail))
    if how == "first":
        return avail[:c]
    if how == "last":
        return avail[len(avail) - c:]
    return np.sort(b.rng.choice(avail, c, replace=False))


def _roles(b, gaps):
    """the queries that are special by VALUE: set before any column is steered"""
    P, n = b.P, b.n
    if n >= 3:
        b.zero = 1
        b.Q[:, 1] = 0
    if b.bits == 16 and n >= 5:
        b.lo_ff, b.hi_ff = 2, 3
        b.Q[:, 2] = (b.rng.integers(0, 0xff, P) << 8) | 0xff                     # (high byte below 0xff: never `empty`)
        b.Q[:, 3] = 0xff00 | b.rng.integers(0, 0xff, P)
    if gaps:
        for q in range(5, n - 1, 3):                                            # `empty` in a third of the rows
            b.Q[b.rng.random(P) < 1 / 3, q] = b.empty
            b.gaps.append(q)


def _steer_lists(b, full_counts, other_counts):
    """the full list (three placements per count, one column equal in EVERY row) for query 0 and the last query, three
    columns for every other; the columns: see planes()"""
    P, n, G, T = b.P, b.n, b.G, b.tile
    cw = 4 if b.bits == 8 else 2                                                # columns per 32-bit word of a row
    chunks = nchunks(P)
    fulls = [0] if n == 1 else [0, n - 1]
    plan = []                                                                   # (q, rows, counts, tag), query 0's first
    for q in fulls:
        for c in full_counts:
            for how in PLACEMENTS:
                plan.append((q, _placed(b, q, c, how), (c,) + (0,) * (chunks - 1), f"{c} {how}"))
        rows = np.flatnonzero(b.Q[:, q] != b.empty)
        plan.append((q, rows, per_chunk(rows, P), "every row"))
    # the places that matter, dealt to query 0's and the last query's columns in turn, largest counts first: a word whose
    # columns are all steered; the last columns of tile 0, the first of tile 1, the very last column
    word0 = list(range(cw))
    places = word0 + [T - 1, T - 2, T, T + 1, G - 1, T - 3, T + 2, G - 2]
    by_size = sorted(range(len(plan)), key=lambda i: (-int(sum(plan[i][2])), i))
    prefer = [c for c in (16368, 256, 255, 4096, 8192, 257, 512, 16367) if c in full_counts]
    prefer += [c for c in sorted(full_counts, reverse=True) if c not in prefer and c > 0]
    chosen = []
    for how in PLACEMENTS:
        for c in prefer:
            for q in fulls:
                chosen.append(next(i for i in range(len(plan)) if plan[i][0] == q and plan[i][3] == f"{c} {how}"))
    chosen = chosen[:len(places)]
    for i, col in zip(chosen, places):
        q, rows, counts, tag = plan[i]
        b.steer(q, col, rows, counts, tag + " @%d" % col)
    # one word per byte position (half): a steered column of query 0 there, columns that match query 0 NOWHERE beside it
    lone = [i for i in by_size if i not in chosen and plan[i][0] == 0 and sum(plan[i][2]) > 0][:cw]
    for k, i in enumerate(lone):
        base = 16 + cw * k
        for j in range(cw):
            if j == k:
                b.steer(0, base + j, plan[i][1], plan[i][2], plan[i][3] + " alone in its word")
            else:
                b.steer(0, base + j, [], (0,) * chunks, "neighbour of a steered column")
    rest = [i for i in range(len(plan)) if i not in chosen and i not in lone]
    for q in range(n):
        if q in fulls:
            continue
        for k, c in enumerate(other_counts):
            how = PLACEMENTS[(q + k) % 3]
            rest.append(len(plan))
            plan.append((q, _placed(b, q, c, how), (c,) + (0,) * (chunks - 1), f"{c} {how}"))
    free = b.free_columns()
    assert len(rest) <= len(free), (len(rest), len(free))
    for i, col in zip(rest, free):
        q, rows, counts, tag = plan[i]
        b.steer(q, col, rows, counts, tag)


@functools.lru_cache(maxsize=None)
def planes(h, bits, n):
    """Every count of COUNTS within chunk 0, three placements each, for query 0 and the last query, 255 / 256 / 4096 for the
    others; steered columns in all (both) places of word 0, at T - 1, T - 2, T - 3 (the end of tile 0), T, T + 1, T + 2 (the
    start of tile 1), G - 1 and G - 2, and alone in words 4 .. 7 (4 .. 5) at every byte position (half) beside columns that
    match nothing.  Query 1 is 0 in every row (n >= 3), queries 5, 8, ... have `empty` in a third of their rows; two bytes
    (n >= 5): query 2 has low byte 0xff throughout, query 3 high byte 0xff."""
    assert h in (14, 15) and bits in (8, 16)
    b = _Build(1 << h, bits, n, 1000 * h + 10 * n + bits)
    _roles(b, gaps=True)
    _steer_lists(b, COUNTS, OTHERS)
    return b.done()


@functools.lru_cache(maxsize=None)
def small(h, bits):
    """P = 8 (the compare kernel), 16 (one block of the table kernel), 256 (the in-loop flush and the final one coincide):
    counts 0, 1, P - 1, P; one octet of queries"""
    assert h in (3, 4, 8)
    P = 1 << h
    b = _Build(P, bits, 8, 77 * h + bits)
    _roles(b, gaps=False)
    _steer_lists(b, (0, 1, P - 1, P), (1, P - 1, P))
    return b.done()


@functools.lru_cache(maxsize=None)
def edges(h=14, bits=8):
    """One octet of queries, columns steered for query 0 only, at the rows where the table kernel's bookkeeping turns over"""
    assert h == 14
    P = 1 << h
    b = _Build(P, bits, 8, 4242 + bits)
    G, T = b.G, b.tile
    rows_of = []
    for i in range(16):                                            # every row position of a block of sixteen weighs exactly one
        rows_of.append((np.arange(i, P, 16), f"rows = {i} mod 16"))
    rows_of += [
        (np.arange(0, 256), "[0, 256): reaches 256 in the last row before the first flush"),
        (np.arange(1, 257), "[1, 257): reaches 256 in the first row after the flush"),
        (np.arange(16, 272), "[16, 272)"),
        (np.arange(4095 - 255, 4096), "[3840, 4096)"),
        (np.arange(CHUNK - 256, CHUNK), "the last 256 rows of chunk 0: the carry is pending when the rows end"),
        (np.arange(CHUNK - 8, CHUNK + 8), "astride the chunk edge"),
        (np.arange(CHUNK, P), "chunk 1 only"),
        (np.array([0]), "row 0"), (np.array([CHUNK - 1]), "row 16,367"), (np.array([CHUNK]), "row 16,368"), (np.array([P - 1]), "the last row"),
    ]
    places = list(range(16)) + [T - 1, T, G - 1, T - 2, T + 1, T - 3, T + 2, G - 2, 20, 25, 30]
    assert len(places) == len(rows_of)
    for (rows, tag), col in zip(rows_of, places):
        b.steer(0, col, rows, per_chunk(rows, P), tag)
    return b.done()


@functools.lru_cache(maxsize=None)
def spill(bits):
    """h = 9, for the compare kernel over ragged windows of rows (its one-byte mismatch counters spill every 248 rows).
    Query 0 is non-empty in every row; five kinds of column for it, next to each other from column 0 (the four byte
    positions of a word and the next word's first), again from column 9 (shifted by one) and at the end of the matrix.
    Query 1 has `empty` in rows [240, 256): a column that matches it in every other row, and one that matches nowhere."""
    P = 512
    b = _Build(P, bits, 8, 909 + bits)
    b.Q[240:256, 1] = b.empty
    b.gaps.append(1)
    rows = np.arange(P)
    kinds = [
        (rows[248:], "nowhere in [0, 248)"),
        (np.concatenate(([100], rows[248:])), "exactly one match in [0, 248)"),
        (rows[408:], "nowhere in [0, 408)"),
        (rows[:0], "nowhere at all"),
        (rows, "everywhere"),
    ]
    for base in (0, 9, b.G - 5):
        for k, (r, tag) in enumerate(kinds):
            b.steer(0, base + k, r, per_chunk(r, P), tag)
    live = np.flatnonzero(b.Q[:, 1] != b.empty)
    b.steer(1, 16, live, per_chunk(live, P), "every row the query has")
    b.steer(1, 17, [], (0,), "nowhere at all")
    return b.done()
