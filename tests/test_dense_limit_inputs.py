"""The inputs of test_gpu_dense_limits.py, proven by the yardstick alone before any GPU is involved (dense_limits.py: plain
numpy): every steered column reaches exactly the count its builder means, chunk by chunk; the counts of query 0 hold the
whole list of limits; bit planes 12 and 13 are each set in some count and clear in another.  And the yardstick is the
reference's definition: count() over an oracle's stored columns is query_sequence of the genomes' sequences."""
import numpy as np
import pytest

import dense_limits as dl

WIDTHS = [8, 16]
# the limits, restated (not read from the builder): both sides of 16 (one block of rows), of 256 (the register planes), of 512, of
# 4,096 and 8,192 (planes 12 and 13), and of a chunk's 16,368 rows
TARGETS = (0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 4095, 4096, 4097, 8191, 8192, 16367, 16368)
CASES = ([("planes", (14, bits, n)) for bits in WIDTHS for n in (8, 16, 24, 72)] +
         [("planes", (15, bits, 16)) for bits in WIDTHS] +
         [("planes", (14, 8, n)) for n in (1, 5, 9, 17, 33, 65)] +
         [("edges", (14, bits)) for bits in WIDTHS] +
         [("small", (h, bits)) for h in (3, 4, 8) for bits in WIDTHS] +
         [("spill", (bits,)) for bits in WIDTHS])


@pytest.fixture(scope="module")
def counted():
    """(Q, M, meta, scores, active, per_chunk) of a case, counted once"""
    made = {}

    def get(name, args):
        if (name, args) not in made:
            Q, M, meta = getattr(dl, name)(*args)
            made[name, args] = (Q, M, meta) + dl.count(Q, M, meta.empty)
        return made[name, args]
    return get


@pytest.mark.parametrize("name,args", CASES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_every_steered_column_reaches_its_count(counted, name, args):
    Q, M, meta, scores, active, per = counted(name, args)
    P, n, G = meta.P, meta.n, meta.G
    assert Q.shape == (P, n) and M.shape == (P, G) and per.shape == (dl.nchunks(P), n, G)
    assert G % meta.tile not in (0,) and G > meta.tile, "two row tiles, the second ragged"
    assert len({s.col for s in meta.steer}) == len(meta.steer)
    for s in meta.steer:
        assert tuple(int(x) for x in per[:, s.q, s.col]) == s.counts, s.tag
        assert s.counts == dl.per_chunk(s.rows, P) and len(s.rows) == sum(s.counts), s.tag
        assert (Q[s.rows, s.q] != meta.empty).all(), s.tag                  # (a row where the query is empty counts for nobody)
    assert ((Q != meta.empty).sum(0) > 0).all(), "no query column is entirely empty"
    np.testing.assert_array_equal(active, (Q != meta.empty).sum(0))
    if meta.zero is not None:
        assert (Q[:, meta.zero] == 0).all()                                 # the query the padding of [G, pitch) matches
    for q in meta.gaps:
        assert (Q[:, q] == meta.empty).any()
    if meta.lo_ff is not None:
        assert ((Q[:, meta.lo_ff] & 0xff) == 0xff).all() and ((Q[:, meta.hi_ff] >> 8) == 0xff).all()
    assert Q.max() <= meta.empty and M.max() <= meta.empty
    assert np.array_equal(dl.to_dump(M, meta.bits).reshape(P, G, meta.bits // 8)[:, :, -1], M & 0xff)   # big-endian: the low byte last


@pytest.mark.parametrize("args", [a for name, a in CASES if name == "planes"], ids=lambda a: "-".join(map(str, a)))
def test_planes_hold_the_whole_list_where_it_matters(counted, args):
    Q, M, meta, scores, active, per = counted("planes", args)
    h, bits, n = args
    P, G, T = meta.P, meta.G, meta.tile
    cw = 32 // bits
    for q in {0, n - 1}:
        mine = [s for s in meta.steer if s.q == q]
        in0 = {int(per[0, q, s.col]) for s in mine}
        assert in0 >= set(TARGETS), sorted(set(TARGETS) - in0)
        for c in TARGETS:                                                 # three placements: the first rows, the last, scattered
            tags = {s.tag.split(" @")[0].replace(" alone in its word", "") for s in mine if s.counts[0] == c and sum(s.counts[1:]) == 0}
            assert tags >= {f"{c} {how}" for how in dl.PLACEMENTS}, (q, c, tags)
        for how, c in (("first", 4096), ("last", 4096)):
            s = next(s for s in mine if s.tag.startswith(f"{c} {how}"))
            assert (s.rows == (np.arange(c) if how == "first" else np.arange(dl.CHUNK - c, dl.CHUNK))).all()
        assert any(int(scores[q, s.col]) == P for s in mine), "a column equal in every row: the sum across chunks"
    for plane in (12, 13):                                                  # the two planes no test set before
        vals = [int(per[0, 0, s.col]) for s in meta.steer if s.q == 0]
        assert any(v >> plane & 1 for v in vals) and any(not v >> plane & 1 for v in vals if v >= 4096), plane
    for q in range(n):
        mine = sorted(int(per[0, q, s.col]) for s in meta.steer if s.q == q)
        assert len(mine) >= 3 and (q in (0, n - 1) or mine == [255, 256, 4096]), (q, mine)
    cols = {s.col for s in meta.steer}
    assert cols >= set(range(cw)) | {T - 1, T - 2, T, T + 1, G - 1}         # a word of steered columns, both sides of the tile edge, the last column
    for k in range(cw):                                                     # alone in its word at byte position (half) k
        word = [s for s in meta.steer if s.col // cw == (16 + cw * k) // cw]
        assert len(word) == cw and all(s.q == 0 for s in word)
        assert [sum(s.counts) > 0 for s in sorted(word, key=lambda s: s.col)] == [j == k for j in range(cw)]
    if n >= 3:
        assert meta.zero == 1
    if n >= 8:
        assert meta.gaps and all(0.25 < (Q[:, q] == meta.empty).mean() < 0.42 for q in meta.gaps)
    if bits == 16 and n >= 5:
        assert (meta.lo_ff, meta.hi_ff) == (2, 3)
    assert dl.nchunks(P) == (2 if h == 14 else 3) and P - (dl.nchunks(P) - 1) * dl.CHUNK == (16 if h == 14 else 32)


@pytest.mark.parametrize("bits", WIDTHS)
def test_near_misses_differ_in_one_field_at_a_time(bits):
    """one byte: each of the eight bits is the only differing one in turn; two bytes: low equal / high equal / swapped"""
    Q, M, meta = dl.edges(14, bits)
    s = next(s for s in meta.steer if s.tag == "row 0")
    q, col = Q[:, 0], M[:, s.col]
    assert col[0] == q[0] and (col[1:] != q[1:]).all()
    x = (col ^ q)[1:]
    if bits == 8:
        assert all(bin(int(v)).count("1") == 1 for v in x[:64]) and {int(v) for v in x[:16]} == {1 << i for i in range(8)}
    else:
        lo_eq, hi_eq = (x & 0xff) == 0, (x >> 8) == 0
        swapped = col[1:] == (((q[1:] & 0xff) << 8) | (q[1:] >> 8))
        assert (lo_eq & ~hi_eq).sum() > 5000 and (hi_eq & ~lo_eq).sum() > 5000 and (swapped & ~lo_eq & ~hi_eq).sum() > 5000
        assert (lo_eq | hi_eq | swapped).all()


@pytest.mark.parametrize("bits", WIDTHS)
def test_edges_and_spill_rows(counted, bits):
    Q, M, meta, scores, active, per = counted("edges", (14, bits))
    by = {s.tag: s for s in meta.steer}
    assert all(s.q == 0 for s in meta.steer) and (Q[:, 0] != meta.empty).all()
    for i in range(16):
        s = by[f"rows = {i} mod 16"]
        assert s.col == i and (s.rows % 16 == i).all() and len(s.rows) == meta.P // 16
    want = {"[0, 256)": (0, 256), "[1, 257)": (1, 257), "[16, 272)": (16, 272), "[3840, 4096)": (3840, 4096), "the last 256": (dl.CHUNK - 256, dl.CHUNK),
            "astride": (dl.CHUNK - 8, dl.CHUNK + 8), "chunk 1 only": (dl.CHUNK, meta.P), "row 0": (0, 1), "row 16,367": (dl.CHUNK - 1, dl.CHUNK),
            "row 16,368": (dl.CHUNK, dl.CHUNK + 1), "the last row": (meta.P - 1, meta.P)}
    for key, (lo, hi) in want.items():
        s = next(s for t, s in by.items() if t.startswith(key))
        assert (s.rows == np.arange(lo, hi)).all(), key
    assert by["astride the chunk edge"].counts == (8, 8) and by["chunk 1 only"].counts == (0, 16)
    Q, M, meta, scores, active, per = counted("spill", (bits,))
    assert meta.P == 512 and (Q[:, 0] != meta.empty).all() and (np.flatnonzero(Q[:, 1] == meta.empty) == np.arange(240, 256)).all()
    kinds = {"nowhere in [0, 248)": 264, "exactly one match in [0, 248)": 265, "nowhere in [0, 408)": 104, "nowhere at all": 0, "everywhere": 512}
    for base in (0, 9, meta.G - 5):
        five = sorted((s for s in meta.steer if s.q == 0 and base <= s.col < base + 5), key=lambda s: s.col)
        assert [(s.tag, int(scores[0, s.col])) for s in five] == list(kinds.items())
    assert not (M[:248, 0] == Q[:248, 0]).any() and (M[:248, 1] == Q[:248, 0]).sum() == 1 and not (M[:408, 2] == Q[:408, 0]).any()
    assert sorted(int(scores[1, s.col]) for s in meta.steer if s.q == 1) == [0, 496] and active[1] == 496


@pytest.mark.parametrize("h", [3, 4, 8])
@pytest.mark.parametrize("bits", WIDTHS)
def test_small_counts(counted, h, bits):
    Q, M, meta, scores, active, per = counted("small", (h, bits))
    P = 1 << h
    assert meta.P == P and meta.n == 8
    for q in (0, 7):
        assert {int(scores[q, s.col]) for s in meta.steer if s.q == q} >= {0, 1, P - 1, P}


@pytest.mark.parametrize("name", ["messy", "w16"])
def test_the_yardstick_is_the_references_definition(name):
    """count() of the stored columns against the stored columns = query_sequence of every indexed genome's sequence
    (test_stored_column_is_the_query.py: a genome's stored column is its gated sketch)"""
    import synth
    from oracle import oracle as orc
    case = synth.CASES[name]()
    seqs = case.genome_sequences()
    o = orc.OracleMiekki(case.k, case.h, case.fp_bits, case.b, case.threshold)
    o.insert_sequences(seqs)
    cols = o.columns()
    G, empty = o.index_size, (1 << case.fp_bits) - 1
    M = cols.astype(np.int64) if o.W == 1 else (cols[:, 0::2].astype(np.int64) << 8) | cols[:, 1::2]
    assert M.shape == (1 << case.h, G)
    np.testing.assert_array_equal(dl.to_dump(M, case.fp_bits).reshape(cols.shape), cols)
    ids = np.arange(G)
    scores, active, _ = dl.count(M[:, ids], M, empty)
    for g, s in enumerate(seqs):
        row, act = o.query_sequence(s)
        np.testing.assert_array_equal(scores[g], row, err_msg=f"{name} genome {g}")
        assert int(active[g]) == act, (name, g)


def plane_counter(eq, flush_blocks=16, final_flush=True):
    """A model of the table kernel's counter for one chunk of rows (eq[rows][columns], rows a multiple of 16): blocks of
    sixteen rows into eight low bits, a carry out of them OR-ed into `pend`, `pend` added to the upper bits every
    flush_blocks blocks and after the last row.  With 16 blocks (256 rows) it counts exactly."""
    blocks = eq.reshape(-1, 16, eq.shape[1]).sum(1)
    low, up, pend = np.zeros(eq.shape[1], np.int64), np.zeros(eq.shape[1], np.int64), np.zeros(eq.shape[1], bool)
    for b in range(len(blocks)):
        low += blocks[b]
        carry = low >= 256
        low -= 256 * carry
        pend |= carry
        if b % flush_blocks == flush_blocks - 1:
            up += pend
            pend[:] = False
    if final_flush:
        up += pend
    return (up * 256 + low) % (1 << 14)


@pytest.mark.parametrize("bits", WIDTHS)
def test_the_inputs_tell_a_late_or_a_lost_flush(counted, bits):
    """What the steered rows are FOR, shown on the model: a flush every 512 rows loses a carry wherever a counter passes two
    multiples of 256 in between (the long runs of `planes`), a missing flush after the last row loses the carry of the
    column that matches in the last 256 rows of the chunk (`edges`) -- and the model as the kernel has it counts exactly."""
    for name, args in (("planes", (14, bits, 8)), ("edges", (14, bits))):
        Q, M, meta, scores, active, per = counted(name, args)
        cols = np.array([s.col for s in meta.steer if s.q == 0])
        eq = (M[:dl.CHUNK, cols] == Q[:dl.CHUNK, :1])
        want = per[0, 0, cols]
        np.testing.assert_array_equal(plane_counter(eq), want)
        late, lost = plane_counter(eq, flush_blocks=32) != want, plane_counter(eq, final_flush=False) != want
        tags = [s.tag for s in meta.steer if s.q == 0]
        if name == "planes":
            assert late.sum() >= 20 and {t.split()[0] for t, x in zip(tags, late) if x} >= {"512", "4096", "8192", "16368"}
            # (the last in-loop flush is behind row 16,127: a run that ends with the chunk passes its last multiple of 256 after it)
            assert {t.split(" @")[0] for t, x in zip(tags, lost) if x} >= {"256 last", "257 last", "512 last", "4096 last"}
        else:
            assert [t for t, x in zip(tags, lost) if x] == ["the last 256 rows of chunk 0: the carry is pending when the rows end"]
