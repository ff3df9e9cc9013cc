"""mk_taxonomy_* / mk_lca_tally_reset / mk_qset_run_lca / mk_lca_tally_read / mk_query_lca and Miekki.lca: every read placed
in a taxonomy by lowest common ancestor on the device must be, counter for counter and read for read, what tests/lca_ref.py
makes of the ORACLE's filter_results -- for five taxonomies, three margins, over u32 scores and over one- and two-byte partial
counts, on tally_ref.Sample as it is and on the grouped collection whose planted runs straddle the walks' steps."""
import ctypes as C

import numpy as np
import pytest

import clade_ref as cr
import lca_ref as lr
import synth
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED, MK_ERR_STATE = 0, -1, -2, -5
THRESHOLDS = [(10, 10.0), (10, 60.0)]
TAXONOMIES = ["flat", "deep", "masked", "single", "empty"]
FEW = 500                          # a set below 512 short reads leaves partial counts, 512 or more u32 scores (test_gpu_tally.slab_reads_check)
G = 1101


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """an input (tally_ref.Sample or lca_ref.Grouped), the oracle's lists of its queries and the placements, each once"""

    def __init__(self, s):
        self.s = s
        self.trees = {name: lr.Tree(nodes, G) for name, nodes in lr.taxonomies(G).items()}
        self.lists, self.memo = {}, {}

    def per_query(self, ms, mi, which="all"):
        if (ms, mi, which) not in self.lists:
            rows = {"all": self.s.rows, "few": self.s.read_rows[:FEW], "genomes": self.s.a.rows}[which]
            self.lists[ms, mi, which] = cr.per_query(self.s.o, rows, ms, mi)
        return self.lists[ms, mi, which]

    def want(self, name, margin, ms, mi, which="all"):
        """(counters, per-read nodes)"""
        if (name, margin, ms, mi, which) not in self.memo:
            self.memo[name, margin, ms, mi, which] = lr.lca_tally(self.per_query(ms, mi, which), self.trees[name], margin)
        return self.memo[name, margin, ms, mi, which]


@pytest.fixture(scope="module")
def sample_index(hip):
    w = Wanted(tr.Sample())
    ix = w.s.a.build(hip)
    yield w, ix
    ix.close()


@pytest.fixture(scope="module")
def grouped_index(hip):
    w = Wanted(lr.Grouped())
    ix = w.s.a.build(hip)
    yield w, ix
    ix.close()


@pytest.fixture(scope="module")
def wide_index(hip):
    """the grouped collection with 16-bit fingerprints: two-byte partial counts"""
    w = Wanted(lr.Grouped(fp_bits=16))
    ix = w.s.a.build(hip)
    yield w, ix
    ix.close()


class DevBuf:
    def __init__(self, ix, nbytes):
        self.ix, self.p = ix, C.c_void_p()
        check(ix._lib.mk_dev_alloc(ix._h, max(nbytes, 64), C.byref(self.p)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ix._lib.mk_dev_free(self.ix._h, self.p)

    def upload(self, arr):
        check(self.ix._lib.mk_dev_upload(self.ix._h, self.p, arr.ctypes.data, arr.nbytes))

    def download(self, arr):
        check(self.ix._lib.mk_dev_download(self.ix._h, arr.ctypes.data, self.p, arr.nbytes))
        return arr


class Uploaded:
    """a set of uploaded sequences"""

    def __init__(self, ix, seqs):
        self.ix, self.qs = ix, C.c_void_p()
        n = len(seqs)
        ptrs, lens = (C.c_char_p * n)(*seqs), (C.c_uint64 * n)(*[len(s) for s in seqs])
        check(ix._lib.mk_qset_upload(ix._h, ptrs, lens, n, C.byref(self.qs)))

    def __enter__(self):
        return self.qs

    def __exit__(self, *a):
        self.ix._lib.mk_qset_free(self.ix._h, self.qs)


class FromIndex(Uploaded):
    def __init__(self, ix, ids):
        self.ix, self.qs = ix, C.c_void_p()
        ids = np.ascontiguousarray(ids, np.uint32)
        check(ix._lib.mk_qset_from_index(ix._h, ids.ctypes.data, len(ids), C.byref(self.qs)))


def make_tax(ix, nodes, n_genomes=None):
    """(status, handle) of mk_taxonomy_create over a list of (lo, hi)"""
    lo = np.array([n[0] for n in nodes], np.uint32)
    hi = np.array([n[1] for n in nodes], np.uint32)
    t = C.c_void_p()
    st = ix._lib.mk_taxonomy_create(ix._h, lo.ctypes.data, hi.ctypes.data, len(nodes), ix.index_size if n_genomes is None else n_genomes, C.byref(t))
    return st, t


class Tax:
    def __init__(self, ix, nodes):
        self.ix = ix
        st, self.t = make_tax(ix, nodes)
        check(st)
        assert ix._lib.mk_taxonomy_nodes(self.t) == len(nodes)

    def __enter__(self):
        return self.t

    def __exit__(self, *a):
        self.ix._lib.mk_taxonomy_free(self.ix._h, self.t)


def run(ix, qs, ms, mi, margin, t, buf, n_slots, node=None):
    return ix._lib.mk_qset_run_lca(ix._h, qs, ms, float(mi), margin, t, buf.p, n_slots, node.p if node else None)


def read(ix, buf, n_slots):
    out = np.full((n_slots, 3), 0xdead, np.uint64)
    check(ix._lib.mk_lca_tally_read(ix._h, buf.p, n_slots, out.ctypes.data))
    return out


def pieces(ix, sets, ms, mi, margin, nodes, passes=1):
    """mk_taxonomy_create, mk_dev_alloc, mk_lca_tally_reset, then per set mk_qset_upload and mk_qset_run_lca `passes` times
    with the set's nodes read back, mk_lca_tally_read: (counters, the sets' per-read nodes one behind the other)"""
    n = len(nodes) + 1
    per_read = []
    with Tax(ix, nodes) as t, DevBuf(ix, 24 * n) as buf:
        check(ix._lib.mk_lca_tally_reset(ix._h, buf.p, n))
        for seqs in sets:
            with Uploaded(ix, seqs) as qs, DevBuf(ix, 4 * len(seqs)) as node:
                node.upload(np.full(len(seqs), 0x5a5a5a5a, np.uint32))
                for _ in range(passes):
                    check(run(ix, qs, ms, mi, margin, t, buf, n, node))
                check(ix._lib.mk_sync(ix._h))
                per_read.append(node.download(np.zeros(len(seqs), np.uint32)))
        return read(ix, buf, n), np.concatenate(per_read)


def same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("ms,mi", THRESHOLDS)
@pytest.mark.parametrize("margin", lr.MARGINS)
@pytest.mark.parametrize("name", TAXONOMIES)
def test_grouped_collection_like_the_oracle(grouped_index, name, margin, ms, mi):
    """the whole mixed set of 628 -- 620 short reads on u32 scores, eight whole genomes on the dense kernel's, so the per-read
    places of a mixed set -- through the pieces and from Python"""
    w, ix = grouped_index
    nodes = w.trees[name].nodes
    want = w.want(name, margin, ms, mi)
    assert (want[0][:, 0].sum() > 0) == (name != "empty")
    same(pieces(ix, [w.s.queries], ms, mi, margin, nodes), want)
    ix.reset_stats()
    got = ix.lca(w.s.queries, nodes, margin, ms, mi, per_read=True)
    assert got[0].dtype == np.uint64 and got[0].shape == want[0].shape and got[1].dtype == np.uint32
    same(got, want)
    if name != "empty":
        assert ix.stats()["filter_ms"] > 0                                  # the lca launches
    np.testing.assert_array_equal(ix.lca(w.s.queries, nodes, margin, ms, mi), want[0])


@pytest.mark.parametrize("margin", lr.MARGINS)
@pytest.mark.parametrize("name", TAXONOMIES)
def test_sample_as_it_is(sample_index, name, margin):
    """tally_ref.Sample: the planted relatives lie at ids 3 ... 1100, so many reads climb to the root"""
    w, ix = sample_index
    for ms, mi in THRESHOLDS:
        same(pieces(ix, [w.s.queries], ms, mi, margin, w.trees[name].nodes), w.want(name, margin, ms, mi))


@pytest.mark.parametrize("margin", lr.MARGINS)
@pytest.mark.parametrize("name", ["deep", "masked"])
def test_one_byte_partial_counts(grouped_index, name, margin):
    """the first 500 reads: a set below 512 short reads is walked over one-byte partial counts"""
    w, ix = grouped_index
    before = ix.stats()["scan_slab_launches"]
    for ms, mi in THRESHOLDS:
        same(pieces(ix, [w.s.reads[:FEW]], ms, mi, margin, w.trees[name].nodes), w.want(name, margin, ms, mi, "few"))
    assert ix.stats()["scan_slab_launches"] > before                       # (partial counts were walked)


@pytest.mark.parametrize("margin", lr.MARGINS)
@pytest.mark.parametrize("name", ["deep", "masked"])
def test_two_byte_partial_counts(wide_index, name, margin):
    """16-bit fingerprints: 512 genomes per tile, the walk over two-byte partial counts; the whole mixed set in one call"""
    w, ix = wide_index
    before = ix.stats()["scan_slab_launches"]
    for ms, mi in THRESHOLDS:
        want = w.want(name, margin, ms, mi, "few")
        assert want[0][:, 0].sum() > 0
        same(pieces(ix, [w.s.reads[:FEW]], ms, mi, margin, w.trees[name].nodes), want)
    assert ix.stats()["scan_slab_launches"] > before
    same(ix.lca(w.s.queries, w.trees[name].nodes, margin, 10, 60.0, per_read=True), w.want(name, margin, 10, 60.0))


def test_sets_from_the_index(grouped_index):
    """every indexed genome as a query from its stored column, in sets of 64 ids, under `deep`: lists of whole species"""
    w, ix = grouped_index
    nodes = w.trees["deep"].nodes
    n = len(nodes) + 1
    with Tax(ix, nodes) as t, DevBuf(ix, 24 * n) as buf, DevBuf(ix, 4 * 64) as node:
        for margin in (10, 100):
            check(ix._lib.mk_lca_tally_reset(ix._h, buf.p, n))
            per_read = []
            for g0 in range(0, G, 64):
                ids = np.arange(g0, min(G, g0 + 64))
                with FromIndex(ix, ids) as qs:
                    check(run(ix, qs, 10, 10.0, margin, t, buf, n, node))
                    check(ix._lib.mk_sync(ix._h))
                    per_read.append(node.download(np.zeros(len(ids), np.uint32)))
            same((read(ix, buf, n), np.concatenate(per_read)), w.want("deep", margin, 10, 10.0, "genomes"))


def test_passes_accumulate_and_sets_leave_no_trace(grouped_index):
    w, ix = grouped_index
    ms, mi, q = 10, 10.0, w.s.queries
    for name, margin in (("deep", 10), ("masked", 0), ("flat", 100)):
        want = w.want(name, margin, ms, mi)
        nodes = w.trees[name].nodes
        same(pieces(ix, [q], ms, mi, margin, nodes, passes=2), (2 * want[0], want[1]))
        same(pieces(ix, [q[:211], q[211:500], q[500:]], ms, mi, margin, nodes), want)


@pytest.mark.parametrize("name,margin", [("deep", 10), ("masked", 100)])
def test_chunks_of_sixteen_queries(grouped_index, monkeypatch, name, margin):
    """the chunks leave no trace: scores and partial counts in chunks of 16 queries, the per-read nodes in their places"""
    w, ix = grouped_index
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "16")
    ms, mi = 10, 10.0
    same(pieces(ix, [w.s.queries], ms, mi, margin, w.trees[name].nodes), w.want(name, margin, ms, mi))
    same(pieces(ix, [w.s.reads[:FEW]], ms, mi, margin, w.trees[name].nodes), w.want(name, margin, ms, mi, "few"))


def test_parents_and_python_refusals(grouped_index):
    w, ix = grouped_index
    from miekki_amd import lib as L
    assert (L.NO_NODE, L.LCA_ABOVE) == (lr.NO_NODE, lr.ABOVE)
    for name in TAXONOMIES:
        tree = w.trees[name]
        with Tax(ix, tree.nodes) as t:
            out = np.full(max(tree.n, 1), 7, np.uint32)
            check(ix._lib.mk_taxonomy_parents(t, out.ctypes.data))
            assert list(out[:tree.n]) == [lr.NO_NODE if p is None else p for p in tree.parent]
    nodes = w.trees["deep"].nodes
    for bad in (101, -1, 2.5, "10", True):
        with pytest.raises(ValueError):
            ix.lca(w.s.queries[:2], nodes, margin=bad)
    with pytest.raises(ValueError):
        ix.lca(w.s.queries[:2], [(0, 5.5)])
    with pytest.raises(ValueError):
        ix.lca(w.s.queries[:2], [(0, -5)])
    with pytest.raises(L.MiekkiHipError) as e:
        ix.lca(w.s.queries[:2], [(5, 9), (0, 4)])
    assert e.value.status == MK_ERR_ARG
    assert ix.lca([], nodes).shape == (len(nodes) + 1, 3) and not ix.lca([], nodes).any()


def test_refusals_leave_the_counters_alone(hip):
    from oracle import oracle as orc
    s = tr.Sample()
    n_g = 200
    short = synth.genome_bases(9, 0, s.c.K)                                 # exactly k long: sketch_size 0
    o = orc.OracleMiekki(*s.c.par)
    o.insert_sequences(s.c.seqs[:n_g] + [short])
    assert o.sketch_size[n_g] == 0
    lists = cr.per_query(o, o.query_sequences(s.queries[:40]), 10, 10.0)
    nodes = [(0, 200), (0, 64), (3, 4), (64, 130), (150, 160)]
    tree = lr.Tree(nodes, n_g + 1)
    want = lr.lca_tally(lists, tree, 100)
    assert want[0].shape == (6, 3) and want[0][:, 0].sum() >= 40
    ix = s.a.build(hip, 0, n_g)
    lib = ix._lib
    try:
        marks = np.arange(3 * 8, dtype=np.uint64).reshape(8, 3)
        out = np.zeros_like(marks)

        def untouched(buf):
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(buf.download(np.zeros_like(marks)), marks)

        # taxonomies that are none: refused on the host, nothing made, the first offending node named
        for bad, says in (([(0, 100), (50, 150)], b"node 1"),                          # an overlap without nesting
                          ([(0, 100), (10, 20), (10, 20)], b"node 2"),                # a duplicate
                          ([(0, 100), (10, 20), (5, 30)], b"node 2"),                 # not in preorder: lo decreases
                          ([(10, 20), (10, 30)], b"node 1"),                          # a child before its parent
                          ([(0, 100), (20, 20)], b"node 1"),                          # empty
                          ([(0, 100), (30, 20)], b"node 1"),
                          ([(0, 100), (150, n_g + 1)], b"node 1")):                   # out of range
            st, t = make_tax(ix, bad)
            assert st == MK_ERR_ARG and t.value is None and says in lib.mk_last_error(), (bad, lib.mk_last_error())
        st, t = make_tax(ix, nodes, n_g - 1)
        assert st == MK_ERR_ARG and t.value is None
        st, t = make_tax(ix, nodes, n_g + 1)
        assert st == MK_ERR_ARG and t.value is None
        lo = np.array([0], np.uint32)
        assert lib.mk_taxonomy_create(ix._h, None, lo.ctypes.data, 1, n_g, C.byref(t)) == MK_ERR_ARG
        assert lib.mk_taxonomy_create(ix._h, lo.ctypes.data, None, 1, n_g, C.byref(t)) == MK_ERR_ARG
        assert lib.mk_taxonomy_create(ix._h, lo.ctypes.data, lo.ctypes.data, 1, n_g, None) == MK_ERR_ARG
        with DevBuf(ix, 24 * 8) as buf, DevBuf(ix, 4 * 40) as node, Uploaded(ix, s.queries[:40]) as qs, Uploaded(ix, []) as none, Tax(ix, nodes) as t, \
                Tax(ix, []) as nothing, FromIndex(ix, np.arange(n_g)) as own:
            buf.upload(marks)
            assert lib.mk_taxonomy_nodes(t) == 5 and lib.mk_taxonomy_nodes(nothing) == 0 and lib.mk_taxonomy_nodes(None) == 0
            mi = C.c_double(10.0)
            assert lib.mk_qset_run_lca(None, qs, 10, mi, 100, t, buf.p, 8, None) == MK_ERR_ARG
            assert lib.mk_qset_run_lca(ix._h, None, 10, mi, 100, t, buf.p, 8, None) == MK_ERR_ARG
            assert lib.mk_qset_run_lca(ix._h, qs, 10, mi, 100, None, buf.p, 8, None) == MK_ERR_ARG
            assert lib.mk_qset_run_lca(ix._h, qs, 10, mi, 100, t, None, 8, None) == MK_ERR_ARG
            assert b"null argument" in lib.mk_last_error()
            assert lib.mk_lca_tally_reset(ix._h, None, 6) == MK_ERR_ARG
            assert lib.mk_lca_tally_read(ix._h, buf.p, 6, None) == MK_ERR_ARG
            assert lib.mk_lca_tally_read(ix._h, None, 6, out.ctypes.data) == MK_ERR_ARG
            assert lib.mk_taxonomy_parents(None, out.ctypes.data) == MK_ERR_ARG
            assert run(ix, qs, 10, 10.0, 100, t, buf, 5) == MK_ERR_ARG      # n_slots = n_nodes: no room for the slot above
            assert b"5 nodes" in lib.mk_last_error()
            assert run(ix, qs, 10, 10.0, 101, t, buf, 8) == MK_ERR_ARG      # the margin
            assert b"margin" in lib.mk_last_error()
            untouched(buf)
            # an empty set, a taxonomy without nodes: MK_OK, the counters as they were, the nodes all MK_NO_NODE
            assert run(ix, none, 10, 10.0, 100, t, buf, 8) == MK_OK
            node.upload(np.full(40, 5, np.uint32))
            assert run(ix, qs, 10, 10.0, 100, nothing, buf, 1, node) == MK_OK
            untouched(buf)
            assert (node.download(np.zeros(40, np.uint32)) == lr.NO_NODE).all()
            # in one call: the same refusals, `out` as it was
            ptrs, lens = (C.c_char_p * 2)(*s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in s.queries[:2]])
            lo, hi = np.array([n[0] for n in nodes], np.uint32), np.array([n[1] for n in nodes], np.uint32)
            assert lib.mk_query_lca(ix._h, ptrs, lens, 2, 10, mi, 101, lo.ctypes.data, hi.ctypes.data, 5, out.ctypes.data, None) == MK_ERR_ARG
            assert lib.mk_query_lca(ix._h, ptrs, lens, 2, 10, mi, 100, None, hi.ctypes.data, 5, out.ctypes.data, None) == MK_ERR_ARG
            assert lib.mk_query_lca(ix._h, ptrs, lens, 2, 10, mi, 100, lo.ctypes.data, hi.ctypes.data, 5, None, None) == MK_ERR_ARG
            assert lib.mk_query_lca(ix._h, None, None, 2, 10, mi, 100, lo.ctypes.data, hi.ctypes.data, 5, out.ctypes.data, None) == MK_ERR_ARG
            assert lib.mk_query_lca(ix._h, ptrs, lens, 2, 10, mi, 100, hi.ctypes.data, lo.ctypes.data, 5, out.ctypes.data, None) == MK_ERR_ARG
            assert not out.any()
            # a genome exactly k long has sketch_size 0: with min_score 0 its intersection is 0 / 0.  It came after the
            # taxonomy was made: the taxonomy leaves it out, the refusal is about the index
            ix.insert_sequences([short])
            assert run(ix, qs, 0, 10.0, 100, t, buf, 8) == MK_ERR_UNSUPPORTED
            assert b"NaN" in lib.mk_last_error()
            assert lib.mk_query_lca(ix._h, ptrs, lens, 2, 0, mi, 100, lo.ctypes.data, hi.ctypes.data, 5, out.ctypes.data, None) == MK_ERR_UNSUPPORTED
            assert not out.any()
            untouched(buf)
            check(run(ix, qs, 10, 10.0, 100, t, buf, 8, node))              # ... and at min_score 10 the pass runs, the new genome left out
            check(lib.mk_sync(ix._h))
            got = buf.download(out.copy()) - marks
            np.testing.assert_array_equal(got[:6], want[0])
            assert not got[6:].any()
            np.testing.assert_array_equal(node.download(np.zeros(40, np.uint32)), want[1])
            buf.upload(marks)
            ix.select(np.arange(n_g))                                       # the k-long genome goes; the taxonomy and `own` name what was there before
            assert run(ix, qs, 10, 10.0, 100, t, buf, 8) == MK_ERR_STATE
            assert b"taxonomy" in lib.mk_last_error()
            with Tax(ix, nodes) as fresh:
                assert run(ix, own, 10, 10.0, 100, fresh, buf, 8) == MK_ERR_STATE   # a stale set, a fresh taxonomy
                untouched(buf)
                check(run(ix, qs, 10, 10.0, 100, fresh, buf, 8))            # ... and an uploaded set runs with it
                check(lib.mk_sync(ix._h))
                np.testing.assert_array_equal((buf.download(out.copy()) - marks)[:6], want[0])
    finally:
        ix.close()


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        t, node = ix.lca(reads, [], per_read=True)
        assert t.shape == (1, 3) and not t.any() and (node == lr.NO_NODE).all()
        m = C.c_void_p()
        assert ix._lib.mk_taxonomy_create(ix._h, None, None, 0, 0, C.byref(m)) == MK_OK and m.value
        marks = np.arange(12, dtype=np.uint64).reshape(4, 3)
        with DevBuf(ix, 96) as buf, DevBuf(ix, 8) as nd, Uploaded(ix, reads) as qs:
            buf.upload(marks)
            nd.upload(np.zeros(2, np.uint32))
            assert run(ix, qs, 10, 10.0, 100, m, buf, 4, nd) == MK_OK
            check(ix._lib.mk_sync(ix._h))
            np.testing.assert_array_equal(buf.download(np.zeros_like(marks)), marks)
            assert (nd.download(np.zeros(2, np.uint32)) == lr.NO_NODE).all()
        ix._lib.mk_taxonomy_free(ix._h, m)
    finally:
        ix.close()
