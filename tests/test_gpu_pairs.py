"""mk_qset_upload_pairs and Miekki.pair_set / pair_scores / query_pairs: a read pair as ONE query.  The yardstick is
tests/pairs_ref.py -- the oracle's minhash_sketch_partition of each mate, the strict-< merge, its check_bloom on the winner,
its stored columns -- at -k 31 -h 9 with 8-bit and -k 31 -h 10 with 16-bit fingerprints.  Everything is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import cover_ref as cv
import pairs_ref as pr
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED = 0, -1, -2
K = pr.K


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


def edge_pairs(seqs):
    """[(what, a, b)]: the kernel's edges, cut from a text of the sample's own genomes so that the gate passes k-mers and
    the scores are not all zero"""
    text = b"".join(seqs[:5])
    assert len(text) > 2 * 4200
    out = []
    # mate lengths around k, every combination
    for L1 in (0, K - 1, K, K + 1, K + 2):
        for L2 in (0, K - 1, K, K + 1, K + 2):
            out.append(("lengths %d %d" % (L1, L2), text[100:100 + L1], pr.revcomp(text[400:400 + L2])))
    # the steps of npad (256, 512, 4,096: per = 1, 2, 16 keys per thread) with the junction at a thread's first key, inside
    # a run of two (odd nk1) and inside a run of sixteen (nk1 = 16 m + 5)
    for nk in (255, 256, 257, 511, 512, 513, 4095, 4096):
        for nk1 in (1, 101, 130, nk - 1):
            assert 101 == 16 * 6 + 5 and 0 < nk1 < nk
            a = text[7:7 + nk1 + K]
            b = pr.revcomp(text[4300:4300 + nk - nk1 + K])
            out.append(("nk %d nk1 %d" % (nk, nk1), a, b))
    # seeds: N and lower case in one mate's k - 1 seed and just past it, the other mate's seed clean
    a, b = text[1000:1150], text[2000:2170]

    def put(s, at, c):
        return s[:at] + c + s[at + 1:]
    for at in (0, K - 2, K - 1):
        out.append(("N at %d of mate 2" % at, a, put(b, at, b"N")))
        out.append(("N at %d of mate 1" % at, put(a, at, b"N"), b))
    out.append(("lower case in mate 2's seed", a, b[:5].lower() + b[5:]))
    out.append(("lower case just past mate 2's seed", a, b[:K - 1] + b[K - 1:K + 3].lower() + b[K + 3:]))
    out.append(("lower case in both", a[:K + 3].lower() + a[K + 3:], b[:K + 3].lower() + b[K + 3:]))
    out.append(("mate 2 = mate 1 with an invalid seed", a, put(a, 3, b"N")))
    out.append(("mate 1 = mate 2 with an invalid seed", put(b, K - 2, b"N"), b))
    # crowded buckets: the bitonic path with a junction
    for L1, L2 in ((300, 260), (1500, 900), (40, 2000)):
        out.append(("repeats %d %d" % (L1, L2), (b"ACGTTGCAT" * 300)[:L1], (b"ACGTTGCAT" * 300)[:L2]))
    # the same with a repeat unit the index holds, so that the gate passes its k-mers: 60 distinct k-mers, dozens of copies each
    unit = text[200:260]
    for L1, L2 in ((1500, 900), (45, 2000), (700, 0)):
        out.append(("indexed repeats %d %d" % (L1, L2), (unit * 40)[:L1], pr.revcomp((unit[17:] + unit * 40)[:L2])))
    return out


class Wanted:
    def __init__(self, bits):
        self.s = pr.Sample(bits)
        self.edges = edge_pairs(self.s.seqs)
        self.edge_rows, self.edge_active = pr.rows(self.s.o, [(a, b) for _, a, b in self.edges], self.s.stored)


@pytest.fixture(scope="module", params=[8, 16])
def work(hip, request):
    w = Wanted(request.param)
    ix = w.s.build(hip)
    yield w, ix
    ix.close()


def mates(pairs):
    return [a for a, _ in pairs], [b for _, b in pairs]


def scores(ix, qs, q0, q1):
    """mk_qset_scores of queries [q0, q1) of a set, with a guard row behind them"""
    G = ix.index_size
    room = np.full((q1 - q0 + 1, G), 0xA5A5A5A5, np.uint32)
    d = C.c_void_p()
    check(ix._lib.mk_dev_alloc(ix._h, room.nbytes, C.byref(d)))
    try:
        check(ix._lib.mk_dev_upload(ix._h, d, room.ctypes.data, room.nbytes))
        check(ix._lib.mk_qset_scores(ix._h, qs, q0, q1, d))
        check(ix._lib.mk_sync(ix._h))
        check(ix._lib.mk_dev_download(ix._h, room.ctypes.data, d, room.nbytes))
    finally:
        ix._lib.mk_dev_free(ix._h, d)
    assert (room[-1] == 0xA5A5A5A5).all()
    return room[:-1]


def active(ix, qs, n):
    out = np.full(n, 0xdead, np.uint32)
    check(ix._lib.mk_qset_active(ix._h, qs, out.ctypes.data))
    return out


def test_the_edges_are_not_trivial_on_the_oracle_alone(work):
    w, _ = work
    rows = {what: r for (what, _, _), r in zip(w.edges, w.edge_rows)}
    assert rows["nk 4096 nk1 101"].max() > 50 and rows["nk 257 nk1 130"].max() > 10
    assert not np.array_equal(rows["N at 0 of mate 2"], rows["N at %d of mate 2" % (K - 1)])
    assert w.edge_active[0] == 0 and w.edge_active.max() > 300
    assert rows["indexed repeats 1500 900"].max() > 5 and rows["repeats 1500 900"].max() == 0


def test_scores_and_active_of_the_sample(work):
    w, ix = work
    a, b = mates(w.s.pairs)
    assert np.array_equal(ix.pair_scores(a, b), w.s.rows)
    with ix.pair_set(a, b) as qs:
        assert np.array_equal(scores(ix, qs, 0, len(a)), w.s.rows)
        assert np.array_equal(active(ix, qs, len(a)), w.s.active)


@pytest.mark.parametrize("nresults", [10, 1, None])
def test_query_pairs_is_filter_results_of_the_yardstick_rows(work, nresults):
    w, ix = work
    o, thr = w.s.o, w.s.par[4]
    a, b = mates(w.s.pairs)
    hits, act = ix.query_pairs(a, b, nresults)
    assert np.array_equal(act, w.s.active)
    listed = 0
    for q, row in enumerate(w.s.rows):
        want = o.filter_results(row, o.index_size if nresults is None else nresults, 10, 0.5 * thr)
        assert [tuple(h) for h in hits[q]] == want, q                      # doubles bit for bit
        listed += len(want)
    assert listed > 200
    # explicit thresholds
    hits, _ = ix.query_pairs(a[:50], b[:50], nresults, min_score=3, min_intersection=2.0)
    for q in range(50):
        assert [tuple(h) for h in hits[q]] == o.filter_results(w.s.rows[q], o.index_size if nresults is None else nresults, 3, 2.0)


def test_kernel_edges_as_one_set(work):
    w, ix = work
    a, b = mates([(x, y) for _, x, y in w.edges])
    got = ix.pair_scores(a, b)
    for i, (what, _, _) in enumerate(w.edges):
        assert np.array_equal(got[i], w.edge_rows[i]), what
    with ix.pair_set(a, b) as qs:
        scores(ix, qs, 0, 1)
        assert np.array_equal(active(ix, qs, len(a)), w.edge_active)


def test_kernel_edges_each_alone(work):
    """a set of one: npad, and with it the keys per thread, is the pair's own"""
    w, ix = work
    for i, (what, a, b) in enumerate(w.edges):
        with ix.pair_set([a], [b]) as qs:
            assert np.array_equal(scores(ix, qs, 0, 1)[0], w.edge_rows[i]), what
            assert int(active(ix, qs, 1)[0]) == int(w.edge_active[i]), what


def test_sub_ranges_invalidate_and_the_mates_swapped(work):
    w, ix = work
    a, b = mates([(x, y) for _, x, y in w.edges])
    n = len(a)
    with ix.pair_set(a, b) as qs:
        for q0, q1 in ((0, 1), (3, 13), (24, 26), (25, 58), (n - 9, n), (n - 1, n), (0, n)):
            assert np.array_equal(scores(ix, qs, q0, q1), w.edge_rows[q0:q1]), (q0, q1)
        check(ix._lib.mk_qset_invalidate(ix._h, qs))
        assert np.array_equal(scores(ix, qs, 0, n), w.edge_rows)
        assert np.array_equal(active(ix, qs, n), w.edge_active)
    # orientation needs no flag: reverse complements of both mates give the same sketch where no seed rule differs
    pa, pb = mates(w.s.pairs[:60])
    assert np.array_equal(ix.pair_scores(pb, pa), pr.rows(w.s.o, list(zip(pb, pa)), w.s.stored)[0])


def test_over_the_limit_and_bad_arguments(work):
    w, ix = work
    text = b"".join(w.s.seqs[:5])
    a, b = text[:2000 + K], text[3000:3000 + 2097 + K]                     # 4,097 k-mers
    ok = (text[:100], text[200:300])
    with pytest.raises(Exception) as e:
        ix.pair_scores([ok[0], ok[0], a], [ok[1], ok[1], b])
    assert e.value.status == MK_ERR_UNSUPPORTED and "pair 2" in str(e.value)
    with pytest.raises(Exception) as e:
        ix.pair_scores([text[:4097 + K]], [b""])                           # one mate alone over the limit
    assert e.value.status == MK_ERR_UNSUPPORTED and "pair 0" in str(e.value)
    assert ix.pair_scores([a[:-1]], [b]).shape == (1, ix.index_size)       # 4,096: taken
    with pytest.raises(ValueError):
        ix.pair_scores([ok[0]], [])
    with pytest.raises(ValueError):
        with ix.pair_set([ok[0]], [ok[1], ok[1]]):
            pass
    with pytest.raises(ValueError):
        ix.query_pairs([], [ok[1]])
    qs = C.c_void_p()
    p, l = (C.c_char_p * 1)(ok[0]), (C.c_uint64 * 1)(len(ok[0]))
    lib = ix._lib
    assert lib.mk_qset_upload_pairs(ix._h, None, l, p, l, 1, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_pairs(ix._h, p, None, p, l, 1, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_pairs(ix._h, p, l, None, l, 1, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_pairs(ix._h, p, l, p, None, 1, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_pairs(ix._h, p, l, p, l, 1, None) == MK_ERR_ARG
    # no pairs at all: an empty set
    assert ix.pair_scores([], []).shape == (0, ix.index_size)
    assert ix.query_pairs([], [])[0] == []


def test_tally_and_cover_through_the_handle(work):
    w, ix = work
    o, thr = w.s.o, w.s.par[4]
    G = ix.index_size
    a, b = mates(w.s.pairs)
    singles = [m for p in w.s.pairs for m in p]
    want = tr.tally(o, w.s.rows, 10, 0.5 * thr)
    want_singles = tr.tally(o, o.query_sequences(singles), 10, 0.5 * thr)
    assert not np.array_equal(want, want_singles)                          # on the yardstick first

    def tally_of(qs):
        d = C.c_void_p()
        check(ix._lib.mk_dev_alloc(ix._h, 32 * G, C.byref(d)))
        try:
            check(ix._lib.mk_tally_reset(ix._h, d, G))
            check(ix._lib.mk_qset_run_tally(ix._h, qs, 10, 0.5 * thr, d, G))
            out = np.full((G, 4), 0xdead, np.uint64)
            check(ix._lib.mk_tally_read(ix._h, d, G, out.ctypes.data))
            return out
        finally:
            ix._lib.mk_dev_free(ix._h, d)

    with ix.pair_set(a, b) as qs:
        assert np.array_equal(tally_of(qs), want)
        # cover: the table of the cells the pairs' gated sketches hold
        seen = pr.seen(o, w.s.pairs)
        d = C.c_void_p()
        check(ix._lib.mk_dev_alloc(ix._h, ix._lib.mk_cover_bytes(ix._h), C.byref(d)))
        try:
            check(ix._lib.mk_cover_reset(ix._h, d))
            check(ix._lib.mk_qset_run_cover(ix._h, qs, d))
            cov, cells = np.full(G, 0xdead, np.uint32), C.c_uint64(0xdead)
            check(ix._lib.mk_cover_count(ix._h, d, cov.ctypes.data, C.byref(cells)))
        finally:
            ix._lib.mk_dev_free(ix._h, d)
        assert np.array_equal(cov, cv.covered(o, seen, w.s.stored))
        assert int(cells.value) == int(seen.sum())
    # the same mates as single reads: another tally, and the unpaired path still the oracle's
    n = len(singles)
    qs = C.c_void_p()
    p, l = (C.c_char_p * n)(*singles), (C.c_uint64 * n)(*[len(s) for s in singles])
    check(ix._lib.mk_qset_upload(ix._h, p, l, n, C.byref(qs)))
    try:
        assert np.array_equal(scores(ix, qs, 0, n), o.query_sequences(singles))
        assert np.array_equal(tally_of(qs), want_singles)
    finally:
        ix._lib.mk_qset_free(ix._h, qs)


@pytest.mark.parametrize("bits", [8, 16])
def test_a_set_sketches_again_as_pairs_when_the_index_grows(hip, bits):
    """64 more genomes: the Bloom filter has changed, and with it the gate's answers"""
    s = pr.Sample(bits)
    more = pr.genomes(64, first=300)
    # reads of the NEW genomes among the pairs: their k-mers pass the gate only afterwards
    pairs = s.pairs[:80] + pr.sample_pairs(more, 40, seed=12)
    a, b = mates(pairs)
    before, active_before = pr.rows(s.o, pairs)
    ix = s.build(hip)
    try:
        with ix.pair_set(a, b) as qs:
            assert np.array_equal(scores(ix, qs, 0, len(a)), before)
            assert np.array_equal(active(ix, qs, len(a)), active_before)
            ix.insert_sequences(more)
            s.o.insert_sequences(more)
            after, active_after = pr.rows(s.o, pairs)
            assert active_after[80:].sum() > active_before[80:].sum() + 1000
            assert np.array_equal(scores(ix, qs, 0, len(a)), after)
            assert np.array_equal(active(ix, qs, len(a)), active_after)
    finally:
        ix.close()
