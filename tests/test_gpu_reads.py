"""mk_qset_upload_reads and Miekki.read_set / read_scores / query_reads: a read cut at its bad bases as ONE query.  The
yardstick is tests/reads_ref.py -- the oracle's minhash_sketch_partition of each segment, the strict-< merge, its check_bloom on
the winner, its stored columns -- at -k 31 -h 9 with 8-bit and -k 31 -h 10 with 16-bit fingerprints.  Everything is compared
exactly."""
import ctypes as C

import numpy as np
import pytest

import cover_ref as cv
import pairs_ref as pr
import reads_ref as rr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED = 0, -1, -2
K, Q = rr.K, rr.MIN_QUAL


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    def __init__(self, bits):
        self.s = s = pr.Sample(bits)
        self.edges = rr.edge_reads(s.seqs)
        self.edge_rows, self.edge_active = rr.rows(s.o, Q, [((r, q),) for _, r, q in self.edges], s.stored)
        self.pairs = rr.edge_pairs(s.seqs)
        self.pair_rows, self.pair_active = rr.rows(s.o, Q, [(a, b) for _, a, b in self.pairs], s.stored)
        self.sample = rr.sample_reads(s.seqs)
        self.sample_rows, self.sample_active = rr.rows(s.o, Q, self.sample, s.stored)
        self.single_rows, self.single_active = rr.rows(s.o, Q, [(a,) for a, _ in self.sample], s.stored)


@pytest.fixture(scope="module", params=[8, 16])
def work(hip, request):
    w = Wanted(request.param)
    ix = w.s.build(hip)
    yield w, ix
    ix.close()


def cols(reads):
    return [r for r, _ in reads], [q for _, q in reads]


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


def test_scores_and_active_of_the_sample(work):
    w, ix = work
    (a, qa), (b, qb) = cols([m1 for m1, _ in w.sample]), cols([m2 for _, m2 in w.sample])
    assert not np.array_equal(w.sample_rows, pr.rows(w.s.o, list(zip(a, b)), w.s.stored)[0])      # the cuts matter, on the yardstick
    assert np.array_equal(ix.read_scores(a, qa, Q, b, qb), w.sample_rows)
    assert np.array_equal(ix.read_scores(a, qa, Q), w.single_rows)
    with ix.read_set(a, qa, Q, b, qb) as qs:
        assert np.array_equal(scores(ix, qs, 0, len(a)), w.sample_rows)
        assert np.array_equal(active(ix, qs, len(a)), w.sample_active)
    with ix.read_set(a, qa, Q) as qs:
        assert np.array_equal(scores(ix, qs, 0, len(a)), w.single_rows)
        assert np.array_equal(active(ix, qs, len(a)), w.single_active)


def test_kernel_edges_as_one_set(work):
    w, ix = work
    r, q = cols([(s, x) for _, s, x in w.edges])
    got = ix.read_scores(r, q, Q)
    for i, (what, _, _) in enumerate(w.edges):
        assert np.array_equal(got[i], w.edge_rows[i]), what
    with ix.read_set(r, q, Q) as qs:
        scores(ix, qs, 0, 1)
        assert np.array_equal(active(ix, qs, len(r)), w.edge_active)


def test_kernel_edges_each_alone(work):
    """a set of one: npad, and with it the keys per thread, is the read's own"""
    w, ix = work
    for i, (what, s, x) in enumerate(w.edges):
        with ix.read_set([s], [x], Q) as qs:
            assert np.array_equal(scores(ix, qs, 0, 1)[0], w.edge_rows[i]), what
            assert int(active(ix, qs, 1)[0]) == int(w.edge_active[i]), what


def test_pair_edges_as_one_set_and_each_alone(work):
    w, ix = work
    (a, qa), (b, qb) = cols([m for _, m, _ in w.pairs]), cols([m for _, _, m in w.pairs])
    got = ix.read_scores(a, qa, Q, b, qb)
    for i, (what, _, _) in enumerate(w.pairs):
        assert np.array_equal(got[i], w.pair_rows[i]), what
    with ix.read_set(a, qa, Q, b, qb) as qs:
        scores(ix, qs, 0, 1)
        assert np.array_equal(active(ix, qs, len(a)), w.pair_active)
    for i, (what, (s1, x1), (s2, x2)) in enumerate(w.pairs):
        with ix.read_set([s1], [x1], Q, [s2], [x2]) as qs:
            assert np.array_equal(scores(ix, qs, 0, 1)[0], w.pair_rows[i]), what
            assert int(active(ix, qs, 1)[0]) == int(w.pair_active[i]), what


def test_min_qual_0_is_the_plain_set_and_the_plain_pairs(work):
    w, ix = work
    (a, qa), (b, qb) = cols([m1 for m1, _ in w.sample]), cols([m2 for _, m2 in w.sample])
    assert np.array_equal(ix.read_scores(a, qa, 0, b, qb), ix.pair_scores(a, b))
    assert np.array_equal(ix.read_scores(a, qa, 0), w.s.o.query_sequences(a))
    r, q = cols([(s, x) for _, s, x in w.edges])
    n = len(r)
    plain = C.c_void_p()
    p, l = (C.c_char_p * n)(*r), (C.c_uint64 * n)(*[len(s) for s in r])
    check(ix._lib.mk_qset_upload(ix._h, p, l, n, C.byref(plain)))
    try:
        with ix.read_set(r, q, 0) as qs:
            assert np.array_equal(scores(ix, qs, 0, n), scores(ix, plain, 0, n))
            assert np.array_equal(active(ix, qs, n), active(ix, plain, n))
    finally:
        ix._lib.mk_qset_free(ix._h, plain)
    # a threshold nothing reaches: no read has a k-mer
    assert not ix.read_scores(a[:20], qa[:20], 93).any()


def test_sub_ranges_and_invalidate(work):
    w, ix = work
    r, q = cols([(s, x) for _, s, x in w.edges])
    n = len(r)
    with ix.read_set(r, q, Q) as qs:
        for q0, q1 in ((0, 1), (3, 13), (24, 26), (25, 58), (n - 9, n), (n - 1, n), (0, n)):
            assert np.array_equal(scores(ix, qs, q0, q1), w.edge_rows[q0:q1]), (q0, q1)
        check(ix._lib.mk_qset_invalidate(ix._h, qs))
        assert np.array_equal(scores(ix, qs, 0, n), w.edge_rows)
        assert np.array_equal(active(ix, qs, n), w.edge_active)


def test_the_limit_and_bad_arguments(work):
    w, ix = work
    text = b"".join(w.s.seqs[:5])
    ok = (text[:100], rr.mask(100, [50]))
    long = text[:4097]
    with pytest.raises(Exception) as e:
        ix.read_scores([ok[0], ok[0], long], [ok[1], ok[1], rr.mask(4097)], Q)
    assert e.value.status == MK_ERR_UNSUPPORTED and "read 2" in str(e.value)
    with pytest.raises(Exception) as e:
        ix.read_scores([ok[0], long[:4000]], [ok[1], rr.mask(4000)], Q, [ok[0], long[:97]], [ok[1], rr.mask(97)])
    assert e.value.status == MK_ERR_UNSUPPORTED and "pair 1" in str(e.value)
    # 4,096 characters in all: taken, and right
    s, x = text[:4096], rr.mask(4096, [1000, 3000])
    assert np.array_equal(ix.read_scores([s], [x], Q), rr.rows(w.s.o, Q, [((s, x),)], w.s.stored)[0])
    s2, x2 = text[5000:5096], rr.mask(96, [40])
    assert np.array_equal(ix.read_scores([s[:4000]], [x[:4000]], Q, [s2], [x2]),
                          rr.rows(w.s.o, Q, [((s[:4000], x[:4000]), (s2, x2))], w.s.stored)[0])
    with pytest.raises(ValueError):
        ix.read_scores([ok[0]], [ok[1][:-1]], Q)
    with pytest.raises(ValueError):
        ix.read_scores([ok[0]], [ok[1]], 94)
    with pytest.raises(ValueError):
        ix.read_scores([ok[0]], [ok[1]], Q, [ok[0]])
    with pytest.raises(ValueError):
        ix.query_reads([ok[0]], [ok[1]], Q, [], [])
    qs = C.c_void_p()
    p, x, l = (C.c_char_p * 1)(ok[0]), (C.c_char_p * 1)(ok[1]), (C.c_uint64 * 1)(100)
    lib = ix._lib
    assert lib.mk_qset_upload_reads(ix._h, None, l, x, None, None, None, 1, Q, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_reads(ix._h, p, None, x, None, None, None, 1, Q, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_reads(ix._h, p, l, None, None, None, None, 1, Q, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_reads(ix._h, p, l, x, None, None, None, 1, Q, None) == MK_ERR_ARG
    for part in ((p, None, None), (None, l, None), (None, None, x), (p, l, None), (p, None, x), (None, l, x)):
        assert lib.mk_qset_upload_reads(ix._h, p, l, x, part[0], part[1], part[2], 1, Q, C.byref(qs)) == MK_ERR_ARG, part
    assert lib.mk_qset_upload_reads(ix._h, p, l, x, None, None, None, 1, 94, C.byref(qs)) == MK_ERR_ARG
    assert lib.mk_qset_upload_reads(ix._h, p, l, x, None, None, None, 1, 93, C.byref(qs)) == MK_OK
    lib.mk_qset_free(ix._h, qs)
    # no reads at all: an empty set
    assert ix.read_scores([], [], Q).shape == (0, ix.index_size)
    assert ix.query_reads([], [], Q)[0] == []


@pytest.mark.parametrize("nresults", [10, None])
def test_query_reads_is_filter_results_of_the_yardstick_rows(work, nresults):
    w, ix = work
    o, thr = w.s.o, w.s.par[4]
    (a, qa), (b, qb) = cols([m1 for m1, _ in w.sample]), cols([m2 for _, m2 in w.sample])
    hits, act = ix.query_reads(a, qa, Q, b, qb, nresults=nresults)
    assert np.array_equal(act, w.sample_active)
    listed = 0
    for q, row in enumerate(w.sample_rows):
        want = o.filter_results(row, o.index_size if nresults is None else nresults, 10, 0.5 * thr)
        assert [tuple(h) for h in hits[q]] == want, q
        listed += len(want)
    assert listed > 30                                                     # (the yardstick's own count: the lists are not all empty)
    hits, act = ix.query_reads(a[:50], qa[:50], Q, nresults=nresults, min_score=3, min_intersection=2.0)
    assert np.array_equal(act, w.single_active[:50])
    for q in range(50):
        assert [tuple(h) for h in hits[q]] == o.filter_results(w.single_rows[q], o.index_size if nresults is None else nresults, 3, 2.0)


def test_cover_through_the_handle(work):
    """one sink: the set is an ordinary one"""
    w, ix = work
    o, G = w.s.o, ix.index_size
    (a, qa), (b, qb) = cols([m1 for m1, _ in w.sample]), cols([m2 for _, m2 in w.sample])
    seen = rr.seen(o, Q, w.sample)
    assert not np.array_equal(seen, pr.seen(o, list(zip(a, b))))
    with ix.read_set(a, qa, Q, b, qb) as qs:
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


def test_a_set_sketches_again_under_the_same_rule_when_the_index_grows(hip):
    """64 more genomes: the Bloom filter has changed, and with it the gate's answers"""
    s = pr.Sample(8)
    more = pr.genomes(64, first=300)
    reads = rr.sample_reads(s.seqs, 60) + rr.sample_reads(more, 40, seed=29)
    (a, qa), (b, qb) = cols([m1 for m1, _ in reads]), cols([m2 for _, m2 in reads])
    before, active_before = rr.rows(s.o, Q, reads)
    ix = s.build(hip)
    try:
        with ix.read_set(a, qa, Q, b, qb) as qs:
            assert np.array_equal(scores(ix, qs, 0, len(a)), before)
            ix.insert_sequences(more)
            s.o.insert_sequences(more)
            after, active_after = rr.rows(s.o, Q, reads)
            assert active_after[60:].sum() > active_before[60:].sum() + 100   # (on the yardstick: the gate's answers did change)
            assert np.array_equal(scores(ix, qs, 0, len(a)), after)
            assert np.array_equal(active(ix, qs, len(a)), active_after)
    finally:
        ix.close()
