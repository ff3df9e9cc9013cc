"""mk_taxonomy_markers / mk_query_taxonomy_markers and Miekki.markers: every held cell credited to the deepest node that contains
all its holders, and those of a node's own cells the sample has seen, must be, count for count, what tests/markers_ref.py makes
of the ORACLE's gated sketches and stored columns -- P = 512 on lca_ref.Grouped (G = 1,101) at one byte and at two, under
every layout of lca_ref.taxonomies -- and of matrices crafted here and imported as they are: the values at the edges of a
range, one slot that every lane meets on, rows of nothing and of nothing shared, holders on both sides of a 16-byte piece and of
the tile edge, left-out genomes that hold what a node holds, and a row that overflows the list of touched slots."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import cover_ref as cr
import dense_limits as dl
import lca_ref as lr
import markers_ref as mr
import synth
import taxon_cover_ref as tcr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MK_OK, MK_ERR_ARG, MK_ERR_STATE = 0, -1, -5
WIDTHS = [8, 16]
TAXONOMIES = ["flat", "deep", "masked", "single", "empty"]
ROWS = [1, 7, 512]
# the settings a worker takes in turn: the defaults, the smallest and the largest range of values (two bytes), no filter, no list
SETTINGS = [{}, {"MIEKKI_MARK_VALUES": "256"}, {"MIEKKI_MARK_VALUES": "16384"}, {"MIEKKI_MARK_FILTER": "0"}, {"MIEKKI_MARK_TOUCHED": "0"}]
G = 1101
RANGE = 8192                               # the default range of values at two bytes


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """lca_ref.Grouped at one width with the oracle's table of all its queries and the yardstick per layout, each once"""

    def __init__(self, bits):
        self.s = s = lr.Grouped(fp_bits=bits)
        self.o, self.bits, self.P, self.empty = s.o, bits, s.o.P, cr.empty_of(s.o)
        self.fps = cr.stored(s.o)
        self.seen = cr.seen(s.o, s.queries)
        self.words = cr.pack(self.seen)
        self.cells = int(self.seen.sum())
        self.nbytes = (self.P << bits) >> 3
        self.nodes = lr.taxonomies(G)
        self.trees = {name: lr.Tree(nodes, G) for name, nodes in self.nodes.items()}
        self.memo = {}

    def want(self, name, seen="seen", key="seen"):
        if (name, key) not in self.memo:
            self.memo[name, key] = mr.node_markers(self.fps, self.empty, self.seen if isinstance(seen, str) else seen, self.trees[name])
            self.memo[name, key].setflags(write=False)
        return self.memo[name, key]


@pytest.fixture(scope="module")
def wanted():
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Wanted(bits)
        return made[bits]
    return get


@pytest.fixture(scope="module")
def indexes(hip, wanted):
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = wanted(bits).s.a.build(hip)
        return wanted(bits), made[bits]
    yield get
    for ix in made.values():
        ix.close()


class DevBuf:
    def __init__(self, ix, nbytes):
        self.ix, self.p, self.nbytes = ix, C.c_void_p(), nbytes
        check(ix._lib.mk_dev_alloc(ix._h, max(nbytes, 32), C.byref(self.p)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ix._lib.mk_dev_free(self.ix._h, self.p)

    def upload(self, arr):
        check(self.ix._lib.mk_dev_upload(self.ix._h, self.p, arr.ctypes.data, arr.nbytes))
        return self


class Table(DevBuf):
    """a cover table of the index's own size, reset, with the set of sequences marked into it"""

    def __init__(self, ix, seqs):
        DevBuf.__init__(self, ix, ix._lib.mk_cover_bytes(ix._h))
        check(ix._lib.mk_cover_reset(ix._h, self.p))
        qs, n = C.c_void_p(), len(seqs)
        ptrs, lens = (C.c_char_p * n)(*seqs), (C.c_uint64 * n)(*[len(s) for s in seqs])
        check(ix._lib.mk_qset_upload(ix._h, ptrs, lens, n, C.byref(qs)))
        try:
            check(ix._lib.mk_qset_run_cover(ix._h, qs, self.p))
        finally:
            ix._lib.mk_qset_free(ix._h, qs)


class Tax:
    def __init__(self, ix, nodes):
        self.ix, self.t = ix, C.c_void_p()
        lo = np.array([n[0] for n in nodes], np.uint32)
        hi = np.array([n[1] for n in nodes], np.uint32)
        check(ix._lib.mk_taxonomy_create(ix._h, lo.ctypes.data, hi.ctypes.data, len(nodes), ix.index_size, C.byref(self.t)))

    def __enter__(self):
        return self.t

    def __exit__(self, *a):
        self.ix._lib.mk_taxonomy_free(self.ix._h, self.t)


def node_markers(ix, nodes, seen_p, extra=0):
    """mk_taxonomy_markers over a fresh taxonomy: (uint64 [n_nodes + 1, 2], cells); `extra` slots beyond stay as they were"""
    nm, cells = np.full((len(nodes) + 1 + extra, 2), 0xdead, np.uint64), C.c_uint64(0xdead)
    with Tax(ix, nodes) as t:
        check(ix._lib.mk_taxonomy_markers(ix._h, t, seen_p, nm.ctypes.data, len(nm), C.byref(cells)))
    assert (nm[len(nodes) + 1:] == 0xdead).all()
    return nm[:len(nodes) + 1], int(cells.value)


@pytest.mark.parametrize("name", TAXONOMIES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_every_layout_like_the_yardstick(indexes, bits, name):
    """through the pieces (a table marked by mk_qset_run_cover, then mk_taxonomy_markers) and in one call (Miekki.markers =
    mk_query_taxonomy_markers); the pass is carried by filter_ms"""
    w, ix = indexes(bits)
    nodes, want = w.nodes[name], w.want(name)
    with Table(ix, w.s.queries) as tab:
        ix.reset_stats()
        nm, cells = node_markers(ix, nodes, tab.p, extra=2)
        if nodes:
            assert ix.stats()["filter_ms"] > 0
    np.testing.assert_array_equal(nm, want)
    assert cells == w.cells
    nm, cells = ix.markers(w.s.queries, nodes)
    assert nm.dtype == np.uint64 and nm.shape == (len(nodes) + 1, 2)
    np.testing.assert_array_equal(nm, want)
    assert cells == w.cells
    nm, cells = ix.markers(None, nodes)                                    # specific alone
    np.testing.assert_array_equal(nm[:, 0], want[:, 0])
    assert not nm[:, 1].any() and cells == 0


@pytest.mark.parametrize("bits", WIDTHS)
def test_identities_on_the_device(indexes, bits):
    """the sums over all slots: the winners' claimed and the taxon cover's held of the root; per node the subtree sums stay
    below the taxon cover, and meet it at the root"""
    w, ix = indexes(bits)
    cov, won, cells, claimed = ix.cover_winners(w.s.queries)
    for name in ("deep", "flat", "single"):                                # every genome has a leaf
        nm, n = ix.markers(w.s.queries, w.nodes[name])
        assert n == cells and int(nm[:, 1].sum()) == claimed, name
    nm, _ = ix.markers(w.s.queries, w.nodes["deep"])
    nc, _ = ix.taxon_cover(w.s.queries, w.nodes["deep"])
    assert int(nm[:, 0].sum()) == int(nc[0, 0]) and not nm[-1].any()
    clade = mr.clade_sums(nm, w.trees["deep"])
    assert (clade <= nc).all() and (clade[0] == nc[0]).all() and (clade[1:, 0] < nc[1:, 0]).any()
    nm, _ = ix.markers(w.s.queries, w.nodes["masked"])
    nc, _ = ix.taxon_cover(w.s.queries, w.nodes["masked"])
    assert (mr.clade_sums(nm, w.trees["masked"]) <= nc).all() and int(nm[-1, 0]) > 0


@pytest.mark.parametrize("bits", WIDTHS)
def test_uploaded_tables(indexes, bits):
    """every bit set: covered = specific -- the bit of `empty` counts for nothing, the rows' zero padding holds no value 0; no
    bit set, or only `empty`'s per row: covered = 0, specific unchanged; a NULL table: specific alone, cells = 0"""
    w, ix = indexes(bits)
    nodes, want = w.nodes["masked"], w.want("masked")
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(np.full(w.nbytes // 4, 0xffffffff, np.uint32))
        nm, cells = node_markers(ix, nodes, tab.p)
        np.testing.assert_array_equal(nm[:, 0], want[:, 0])
        np.testing.assert_array_equal(nm[:, 1], want[:, 0])
        assert cells == w.P << bits
        tab.upload(np.zeros(w.nbytes // 4, np.uint32))
        nm, cells = node_markers(ix, nodes, tab.p)
        np.testing.assert_array_equal(nm[:, 0], want[:, 0])
        assert not nm[:, 1].any() and cells == 0
        only_empty = np.zeros((w.P, 1 << bits), bool)
        only_empty[:, w.empty] = True
        tab.upload(cr.pack(only_empty))
        nm, cells = node_markers(ix, nodes, tab.p)
        np.testing.assert_array_equal(nm[:, 0], want[:, 0])
        assert not nm[:, 1].any() and cells == w.P
    nm, cells = node_markers(ix, nodes, None)
    np.testing.assert_array_equal(nm[:, 0], want[:, 0])
    assert not nm[:, 1].any() and cells == 0


@pytest.fixture(scope="module")
def switched(wanted, tmp_path_factory):
    """mk_taxonomy_markers of every layout over the yardstick's table in fresh processes (tests/markers_worker.py), one per
    width and MIEKKI_MARK_ROWS, all six at once; each takes SETTINGS in turn"""
    d = tmp_path_factory.mktemp("markers_switches")
    procs = {}
    for bits in WIDTHS:
        w = wanted(bits)
        with open(d / f"job_{bits}.pkl", "wb") as f:
            pickle.dump({"par": w.s.par, "seqs": w.s.seqs, "words": w.words, "taxonomies": w.nodes, "switches": SETTINGS}, f)
        for rows in ROWS:
            env = dict(os.environ, MIEKKI_MARK_ROWS=str(rows))
            for name in ("MIEKKI_MARK_VALUES", "MIEKKI_MARK_FILTER", "MIEKKI_MARK_TOUCHED"):
                env.pop(name, None)
            procs[bits, rows] = subprocess.Popen([sys.executable, os.path.join(HERE, "markers_worker.py"), str(d / f"job_{bits}.pkl"),
                                                  str(d / f"out_{bits}_{rows}.npz")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for (bits, rows), p in procs.items():
        text = p.communicate(timeout=300)[0]
        assert p.returncode == 0, text.decode(errors="replace")[-3000:]
        out[bits, rows] = dict(np.load(d / f"out_{bits}_{rows}.npz"))
    return out


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=["defaults", "values256", "values16384", "nofilter", "notouched"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("bits", WIDTHS)
def test_switches_give_identical_results(wanted, switched, bits, rows, setting):
    """rows per workgroup 1, 7 and 512 (more than one row per workgroup is what catches a slot that is not cleared between
    rows); the smallest and the largest range of values; the atomics without their filter; the whole range read out"""
    w, got = wanted(bits), switched[bits, rows]
    for name in TAXONOMIES:
        np.testing.assert_array_equal(got["%d/%s" % (setting, name)], w.want(name), err_msg=name)
        assert int(got["%d/%s/cells" % (setting, name)]) == w.cells


# ---- crafted matrices, imported as they are
def import_matrix(ix, M, bits):
    P, n = M.shape
    empty = (1 << bits) - 1
    cols = dl.to_dump(M, bits)
    ss = (M != empty).sum(0).astype(np.uint32)
    gs = np.full(n, 100_000, np.uint64)
    check(ix._lib.mk_index_import_begin(ix._h, n))
    check(ix._lib.mk_index_import_columns(ix._h, 0, P, cols.ctypes.data))
    check(ix._lib.mk_index_import_sizes(ix._h, gs.ctypes.data, ss.ctypes.data))
    assert ix._lib.mk_index_size(ix._h) == n


def crafted(bits):
    """P = 512, G = 1,101: the rows the docstring of this file lists, then rows of few values that many genomes share (every
    owner of the layouts turns up, in batches of one and of many), rows of random values and sparse rows"""
    empty = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    M = np.full((512, G), empty, np.int64)
    rng_edge = RANGE if bits == 16 else 64                                 # one byte: the edge of a lane's slots in the read-out
    edge = [0, 1, rng_edge - 1, rng_edge, empty - 1]
    for i, v in enumerate(edge):
        M[i, [0, G - 1]] = v                                               # the first and the last genome: the root's, or above a forest
        M[5 + i, G - 1] = v                                                # the last genome alone
    M[10, :] = 7                                                           # one slot, 1,101 lanes meet on it
    #   row 11: nothing
    M[12, :] = np.arange(G) * 59 % empty if bits == 16 else np.where(np.arange(G) < empty, np.arange(G), empty)   # no two genomes agree
    for i, (a, b) in enumerate([(7, 8), (15, 16), (511, 512), (1023, 1024)]):
        M[13 + i, [a, b]] = 300 % empty                                    # both sides of a 16-byte piece, of the tile edge
    M[17, 254:259] = 9                                                     # a node's genomes, and genomes that `masked` leaves out
    M[17, [0, 50, 99]] = 9
    M[18, [4, 5]] = 9                                                      # (4, 6): inside one lane
    M[18, [1000, 1100]] = 11                                               # two singleton leaves: their parent's
    for r in range(19, 200):                                               # few values, runs of genomes: owners of every depth
        cut = np.sort(rng.integers(0, G, 40))
        M[r] = rng.integers(0, 6, 41)[np.searchsorted(cut, np.arange(G), side="right")] + (r % 3) * (rng_edge - 3)
    M[200:400] = rng.integers(0, empty, (200, G))
    sparse = rng.integers(0, empty, (112, G))
    M[400:] = np.where(rng.random((112, G)) < 0.02, sparse, empty)
    return M


@pytest.fixture(scope="module")
def crafted_contexts(hip):
    made = {}

    def get(bits):
        if bits not in made:
            ix = hip.Miekki(15, 9, bits, 32, 20)                           # (k, the filter and the threshold play no part: nothing is sketched)
            M = crafted(bits)
            import_matrix(ix, M, bits)
            seen = np.random.default_rng(bits + 1).random((512, 1 << bits)) < 0.5
            made[bits] = (ix, M, seen)
        return made[bits]
    yield get
    for ix, _, _ in made.values():
        ix.close()


@pytest.mark.parametrize("setting", [{}, {"MIEKKI_MARK_ROWS": "3", "MIEKKI_MARK_VALUES": "256"}, {"MIEKKI_MARK_TOUCHED": "0", "MIEKKI_MARK_ROWS": "5"}],
                         ids=["defaults", "rows3_values256", "notouched_rows5"])
@pytest.mark.parametrize("name", ["flat", "deep", "masked", "single"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_crafted_matrices(crafted_contexts, monkeypatch, bits, name, setting):
    ix, M, seen = crafted_contexts(bits)
    empty = (1 << bits) - 1
    nodes = lr.taxonomies(G)[name]
    tree = lr.Tree(nodes, G)
    want = mr.node_markers(M, empty, seen, tree)
    if name != "masked":
        # what the first rows are there for, by the yardstick: a cell per row but for row 11, none, and row 12, a cell per holder
        few = mr.node_markers(M[:18], empty, None, tree)
        assert int(few[:, 0].sum()) == 10 + 1 + (G if bits == 16 else empty) + 4 + 1
    else:
        only = mr.node_markers(M[17:18], empty, None, tree)
        assert int(only[nodes.index((254, 259)), 0]) == 1 and int(only[:, 0].sum()) == 1   # the left-out holders do not move it
    for k, v in setting.items():
        monkeypatch.setenv(k, v)
    with DevBuf(ix, (512 << bits) >> 3) as tab:
        tab.upload(cr.pack(seen))
        nm, cells = node_markers(ix, nodes, tab.p)
    np.testing.assert_array_equal(nm, want)
    assert cells == int(seen.sum())


def test_a_row_that_overflows_the_touched_list(hip, monkeypatch):
    """two bytes, 4,096 genomes: a row in which every genome holds a value of its own inside one range lists 4,096 slots, twice
    the list's 2,048 -- the whole range is read out; the row before and the row after it go by the list"""
    bits, n, empty = 16, 4096, 65535
    rng = np.random.default_rng(4096)
    M = rng.integers(0, 12, (512, n)).astype(np.int64) * 3000              # few values per row, over five ranges
    for r in (1, 200, 511):
        M[r] = rng.permutation(RANGE)[:n] + (RANGE if r == 200 else 0)      # 4,096 values of one range
    M[300] = rng.permutation(empty)[:n]                                     # 4,096 values over all ranges: 512 per range, by the list
    nodes = lr.preorder([(0, n), (0, 2048), (100, 200), (150, 160), (2048, 4096), (2048, 2049), (4000, 4096)])
    tree = lr.Tree(nodes, n)
    seen = rng.random((512, 1 << bits)) < 0.5
    want = mr.node_markers(M, empty, seen, tree)
    ix = hip.Miekki(15, 9, bits, 32, 20)
    try:
        import_matrix(ix, M, bits)
        with DevBuf(ix, (512 << bits) >> 3) as tab:
            tab.upload(cr.pack(seen))
            for rows in (None, "1"):
                if rows:
                    monkeypatch.setenv("MIEKKI_MARK_ROWS", rows)
                nm, cells = node_markers(ix, nodes, tab.p)
                np.testing.assert_array_equal(nm, want)
    finally:
        ix.close()


def test_genomes_appended_after_the_taxonomy_are_left_out(hip, wanted):
    w = wanted(8)
    n_g = 300
    ix = w.s.a.build(hip, 0, n_g)
    try:
        nodes = [(0, n_g), (4, 6), (254, 259)]
        tree = lr.Tree(nodes, n_g)
        with DevBuf(ix, w.nbytes) as tab, Tax(ix, nodes) as t:
            tab.upload(w.words)
            ix.insert_sequences(w.s.seqs[n_g:n_g + 40])                    # the taxonomy stays good: the ids name the same genomes
            nm, cells = np.zeros((4, 2), np.uint64), C.c_uint64(0)
            check(ix._lib.mk_taxonomy_markers(ix._h, t, tab.p, nm.ctypes.data, 4, C.byref(cells)))
        np.testing.assert_array_equal(nm, mr.node_markers(w.fps[:, :n_g + 40], w.empty, w.seen, tree))
    finally:
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_cold_rows_raw_and_packed(hip, wanted, monkeypatch, bits):
    """1 MiB of a 2 MiB matrix in HBM (a reservation doubles the rows' pitch), the other rows in host memory: read where they
    lie; then packed (compress_index), which the pass unpacks first"""
    w = wanted(bits)
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = hip.Miekki(*w.s.par)
    try:
        ix.reserve(4096 * 8 // bits)
        for i in range(0, G, 64):
            ix.insert_sequences(w.s.seqs[i:i + 64])
        nm, cells = ix.markers(w.s.queries, w.nodes["deep"])
        np.testing.assert_array_equal(nm, w.want("deep"))
        assert cells == w.cells
        raw, packed = ix.compress_index()
        assert raw >= 1 << 20                                              # (there are cold rows)
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.words)
            nm, cells = node_markers(ix, w.nodes["masked"], tab.p)         # (unpacks)
            np.testing.assert_array_equal(nm, w.want("masked"))
    finally:
        ix.close()


def test_a_stale_taxonomy_is_refused(hip, wanted):
    w = wanted(8)
    n_g = 200
    ix = w.s.a.build(hip, 0, n_g + 1)
    try:
        lib = ix._lib
        nodes = [(0, n_g + 1), (4, 6)]
        nm, cells = np.full((3, 2), 7, np.uint64), C.c_uint64(7)
        with DevBuf(ix, w.nbytes) as tab, Tax(ix, nodes) as t:
            tab.upload(w.words)
            check(lib.mk_taxonomy_markers(ix._h, t, tab.p, nm.ctypes.data, 3, C.byref(cells)))
            np.testing.assert_array_equal(nm, mr.node_markers(w.fps[:, :n_g + 1], w.empty, w.seen, lr.Tree(nodes, n_g + 1)))
            nm[:], cells.value = 7, 7
            ix.select(np.arange(n_g))                                      # the last genome goes: the taxonomy names what was there before
            assert lib.mk_taxonomy_markers(ix._h, t, tab.p, nm.ctypes.data, 3, C.byref(cells)) == MK_ERR_STATE
            assert b"taxonomy" in lib.mk_last_error()
            assert (nm == 7).all() and cells.value == 7
    finally:
        ix.close()


@pytest.mark.parametrize("switch,value", [("MIEKKI_MARK_ROWS", "0"), ("MIEKKI_MARK_ROWS", "many"), ("MIEKKI_MARK_VALUES", "128"),
                                          ("MIEKKI_MARK_VALUES", "32768"), ("MIEKKI_MARK_VALUES", "300"), ("MIEKKI_MARK_VALUES", "4096x"),
                                          ("MIEKKI_MARK_FILTER", "2"), ("MIEKKI_MARK_FILTER", "off"), ("MIEKKI_MARK_TOUCHED", "-1")])
@pytest.mark.parametrize("bits", WIDTHS)
def test_a_bad_switch_is_refused(indexes, monkeypatch, bits, switch, value):
    w, ix = indexes(bits)
    lib, nodes = ix._lib, w.nodes["deep"]
    monkeypatch.setenv(switch, value)
    nm, cells = np.full((len(nodes) + 1, 2), 7, np.uint64), C.c_uint64(7)
    lo = np.array([n[0] for n in nodes], np.uint32)
    hi = np.array([n[1] for n in nodes], np.uint32)
    ptrs, lens = (C.c_char_p * 2)(*w.s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in w.s.queries[:2]])
    with DevBuf(ix, w.nbytes) as tab, Tax(ix, nodes) as t:
        tab.upload(w.words)
        assert lib.mk_taxonomy_markers(ix._h, t, tab.p, nm.ctypes.data, len(nm), C.byref(cells)) == MK_ERR_ARG
        assert switch.encode() in lib.mk_last_error()
        assert lib.mk_query_taxonomy_markers(ix._h, ptrs, lens, 2, lo.ctypes.data, hi.ctypes.data, len(nodes), nm.ctypes.data, len(nm),
                                             C.byref(cells)) == MK_ERR_ARG
        assert switch.encode() in lib.mk_last_error()
    assert (nm == 7).all() and cells.value == 7


def test_refusals_leave_the_outputs_alone(hip, indexes):
    w, ix = indexes(8)
    lib, nodes = ix._lib, w.nodes["deep"]
    n = len(nodes) + 1
    nm, cells = np.full((n, 2), 7, np.uint64), C.c_uint64(7)
    lo = np.array([x[0] for x in nodes], np.uint32)
    hi = np.array([x[1] for x in nodes], np.uint32)
    ptrs, lens = (C.c_char_p * 2)(*w.s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in w.s.queries[:2]])
    other = hip.Miekki(*w.s.par)
    try:
        with DevBuf(ix, w.nbytes) as tab, Tax(ix, nodes) as t:
            tab.upload(w.words)
            out, pc = nm.ctypes.data, C.byref(cells)
            for args in ((None, t, tab.p, out, n, pc), (ix._h, None, tab.p, out, n, pc), (ix._h, t, tab.p, None, n, pc)):
                assert lib.mk_taxonomy_markers(*args) == MK_ERR_ARG
                assert b"null argument" in lib.mk_last_error()
            assert lib.mk_taxonomy_markers(ix._h, t, tab.p, out, n - 1, pc) == MK_ERR_ARG       # no room for the slot above
            assert b"slot" in lib.mk_last_error()
            assert lib.mk_taxonomy_markers(other._h, t, tab.p, out, n, pc) == MK_ERR_ARG
            assert b"another context" in lib.mk_last_error()
            a = (lo.ctypes.data, hi.ctypes.data, len(nodes))
            assert lib.mk_query_taxonomy_markers(None, ptrs, lens, 2, *a, out, n, pc) == MK_ERR_ARG
            assert lib.mk_query_taxonomy_markers(ix._h, None, None, 2, *a, out, n, pc) == MK_ERR_ARG
            assert lib.mk_query_taxonomy_markers(ix._h, ptrs, lens, 2, None, hi.ctypes.data, len(nodes), out, n, pc) == MK_ERR_ARG
            assert lib.mk_query_taxonomy_markers(ix._h, ptrs, lens, 2, *a, None, n, pc) == MK_ERR_ARG
            assert lib.mk_query_taxonomy_markers(ix._h, ptrs, lens, 2, *a, out, n - 1, pc) == MK_ERR_ARG
            swapped = (hi.ctypes.data, lo.ctypes.data, len(nodes))         # empty intervals: the taxonomy's own refusal
            assert lib.mk_query_taxonomy_markers(ix._h, ptrs, lens, 2, *swapped, out, n, pc) == MK_ERR_ARG
            check(lib.mk_sync(ix._h))
            assert (nm == 7).all() and cells.value == 7
            check(lib.mk_taxonomy_markers(ix._h, t, tab.p, out, n, None))                      # cells may be NULL
            np.testing.assert_array_equal(nm, w.want("deep"))
    finally:
        other.close()


def test_empty_index_and_no_nodes(hip, indexes):
    """an empty index, and a taxonomy without nodes over a full one: MK_OK, the slot above every node written as zero"""
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        nm, cells = ix.markers(reads, [])
        assert nm.shape == (1, 2) and not nm.any() and cells == 0
        out, n = np.full((2, 2), 9, np.uint64), C.c_uint64(99)
        with DevBuf(ix, 16384) as tab, Tax(ix, []) as t:
            tab.upload(np.arange(4096, dtype=np.uint32))
            assert ix._lib.mk_taxonomy_markers(ix._h, t, tab.p, out.ctypes.data, 2, C.byref(n)) == MK_OK
            assert not out[0].any() and (out[1] == 9).all()
            assert ix._lib.mk_taxonomy_markers(ix._h, t, tab.p, out.ctypes.data, 0, C.byref(n)) == MK_ERR_ARG
    finally:
        ix.close()
    w, full = indexes(8)
    nm, cells = full.markers(w.s.queries, [])
    assert nm.shape == (1, 2) and not nm.any() and cells == w.cells
