"""mk_taxonomy_cover / mk_query_taxonomy_cover and Miekki.taxon_cover: per node of a taxonomy the distinct cells its genomes hold
and those of them the sample has seen must be, count for count, what tests/taxon_cover_ref.py makes of the ORACLE's gated
sketches and stored columns -- P = 512 on lca_ref.Grouped (G = 1,101) at one byte and at two, under every layout of
lca_ref.taxonomies: (254, 259) across the 256 step, (4, 6) inside one lane's 16 bytes, (510, 514) unaligned at both ends,
(100, 1050) and the root over the ragged second tile and the padding, 1,101 singletons, a forest, left-out genomes, no node."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import cover_ref as cr
import lca_ref as lr
import synth
import taxon_cover_ref as tcr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MK_OK, MK_ERR_ARG, MK_ERR_STATE = 0, -1, -5
WIDTHS = [8, 16]
TAXONOMIES = ["flat", "deep", "masked", "single", "empty"]
ROWS = [1, 7, 512]
WIDES = [2, None, 2000]
G = 1101


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
        self.o, self.bits, self.P = s.o, bits, s.o.P
        self.fps = cr.stored(s.o)
        self.seen = cr.seen(s.o, s.queries)
        self.words = cr.pack(self.seen)
        self.cells = int(self.seen.sum())
        self.nbytes = (self.P << bits) >> 3
        self.nodes = lr.taxonomies(G)
        self.memo = {}

    def want(self, name, seen=None, key="seen"):
        if (name, key) not in self.memo:
            self.memo[name, key] = tcr.node_cover(self.o, self.seen if seen is None else seen, self.fps, self.nodes[name])
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
    """a cover table of the index's own size, reset, with the sets of sequences given marked into it one after the other"""

    def __init__(self, ix, *sets):
        DevBuf.__init__(self, ix, ix._lib.mk_cover_bytes(ix._h))
        check(ix._lib.mk_cover_reset(ix._h, self.p))
        for seqs in sets:
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


def node_cover(ix, nodes, seen_p):
    """mk_taxonomy_cover over a fresh taxonomy: (uint64 [n_nodes, 2], cells)"""
    nc, cells = np.full((len(nodes), 2), 0xdead, np.uint64), C.c_uint64(0xdead)
    with Tax(ix, nodes) as t:
        check(ix._lib.mk_taxonomy_cover(ix._h, t, seen_p, nc.ctypes.data, C.byref(cells)))
    return nc, int(cells.value)


@pytest.mark.parametrize("name", TAXONOMIES)
@pytest.mark.parametrize("bits", WIDTHS)
def test_every_layout_like_the_yardstick(indexes, bits, name):
    """through the pieces (a table marked by mk_qset_run_cover, then mk_taxonomy_cover) and in one call (Miekki.taxon_cover =
    mk_query_taxonomy_cover); the passes are carried by filter_ms"""
    w, ix = indexes(bits)
    nodes, want = w.nodes[name], w.want(name)
    with Table(ix, w.s.queries) as tab:
        ix.reset_stats()
        nc, cells = node_cover(ix, nodes, tab.p)
        if nodes:
            assert ix.stats()["filter_ms"] > 0
    np.testing.assert_array_equal(nc, want)
    assert cells == w.cells
    nc, cells = ix.taxon_cover(w.s.queries, nodes)
    assert nc.dtype == np.uint64 and nc.shape == (len(nodes), 2)
    np.testing.assert_array_equal(nc, want)
    assert cells == w.cells
    assert (nc[:, 1] <= nc[:, 0]).all()


@pytest.mark.parametrize("bits", WIDTHS)
def test_identities_on_the_device(indexes, bits):
    """a node of one genome: sketch_size and mk_cover_count's covered; the root: mk_cover_winners' claimed"""
    w, ix = indexes(bits)
    cov, won, cells, claimed = ix.cover_winners(w.s.queries)
    nc, n = ix.taxon_cover(w.s.queries, w.nodes["single"])
    assert n == cells and int(nc[0, 1]) == claimed
    np.testing.assert_array_equal(nc[1:, 0], ix.sketch_size)
    np.testing.assert_array_equal(nc[1:, 1], cov)


@pytest.mark.parametrize("bits", WIDTHS)
def test_uploaded_tables(indexes, bits):
    """every bit set: covered = held -- the bit of `empty` counts for nothing, the rows' zero padding holds no value 0; no bit
    set, or only `empty`'s per row: covered = 0, held unchanged; a NULL table: held alone, cells = 0"""
    w, ix = indexes(bits)
    nodes, want = w.nodes["deep"], w.want("deep")
    ones = np.ones((w.P, 1 << bits), bool)
    live = w.fps != cr.empty_of(w.o)
    held = np.zeros((w.P, 1 << bits), bool)
    held[np.nonzero(live)[0], w.fps[live]] = True
    assert held[:, 0].sum() < w.P                                          # some row holds no 0: its padding must not hold (p, 0)
    full = w.want("deep", ones, "ones")
    np.testing.assert_array_equal(full[:, 0], full[:, 1])
    np.testing.assert_array_equal(full[:, 0], want[:, 0])
    assert int(full[0, 0]) == held.sum()
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(np.full(w.nbytes // 4, 0xffffffff, np.uint32))
        nc, cells = node_cover(ix, nodes, tab.p)
        np.testing.assert_array_equal(nc, full)
        assert cells == w.P << bits
        tab.upload(np.zeros(w.nbytes // 4, np.uint32))
        nc, cells = node_cover(ix, nodes, tab.p)
        np.testing.assert_array_equal(nc[:, 0], want[:, 0])
        assert not nc[:, 1].any() and cells == 0
        only_empty = np.zeros((w.P, 1 << bits), bool)
        only_empty[:, cr.empty_of(w.o)] = True
        tab.upload(cr.pack(only_empty))
        nc, cells = node_cover(ix, nodes, tab.p)
        np.testing.assert_array_equal(nc[:, 0], want[:, 0])
        assert not nc[:, 1].any() and cells == w.P
    nc, cells = node_cover(ix, nodes, None)
    np.testing.assert_array_equal(nc[:, 0], want[:, 0])
    assert not nc[:, 1].any() and cells == 0


@pytest.fixture(scope="module")
def switched(wanted, tmp_path_factory):
    """mk_taxonomy_cover of every layout over the yardstick's table in fresh processes (tests/taxon_cover_worker.py), one per
    width and MIEKKI_TAXCOVER_ROWS, all six at once; each takes the three MIEKKI_TAXCOVER_WIDE in turn"""
    d = tmp_path_factory.mktemp("taxon_cover_switches")
    procs = {}
    for bits in WIDTHS:
        w = wanted(bits)
        with open(d / f"job_{bits}.pkl", "wb") as f:
            pickle.dump({"par": w.s.par, "seqs": w.s.seqs, "words": w.words, "taxonomies": w.nodes, "wides": WIDES}, f)
        for rows in ROWS:
            env = dict(os.environ, MIEKKI_TAXCOVER_ROWS=str(rows))
            env.pop("MIEKKI_TAXCOVER_WIDE", None)
            procs[bits, rows] = subprocess.Popen([sys.executable, os.path.join(HERE, "taxon_cover_worker.py"), str(d / f"job_{bits}.pkl"),
                                                  str(d / f"out_{bits}_{rows}.npz")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for (bits, rows), p in procs.items():
        text = p.communicate(timeout=300)[0]
        assert p.returncode == 0, text.decode(errors="replace")[-3000:]
        out[bits, rows] = dict(np.load(d / f"out_{bits}_{rows}.npz"))
    return out


@pytest.mark.parametrize("wide", WIDES)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("bits", WIDTHS)
def test_row_chunks_and_paths_give_identical_results(wanted, switched, bits, rows, wide):
    """rows per item 1, 7 and 512 (at two bytes more than one row per item is what catches a set that is not emptied between
    rows); every node down the wide path (2), by the default width, every node down the narrow path (2,000 > G)"""
    w, got = wanted(bits), switched[bits, rows]
    for name in TAXONOMIES:
        np.testing.assert_array_equal(got["%s/%s" % (wide, name)], w.want(name), err_msg=name)
        assert int(got["%s/%s/cells" % (wide, name)]) == w.cells


@pytest.mark.parametrize("bits", WIDTHS)
def test_results_do_not_depend_on_how_the_reads_are_split(indexes, bits):
    w, ix = indexes(bits)
    q = w.s.queries
    half = len(q) // 2
    with Table(ix, q[:half], q[half:]) as tab:                             # halves
        nc, cells = node_cover(ix, w.nodes["deep"], tab.p)
    np.testing.assert_array_equal(nc, w.want("deep"))
    assert cells == w.cells
    with Table(ix, q, q) as tab:                                           # the set twice
        nc, cells = node_cover(ix, w.nodes["deep"], tab.p)
    np.testing.assert_array_equal(nc, w.want("deep"))
    assert cells == w.cells


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
        nc, cells = ix.taxon_cover(w.s.queries, w.nodes["deep"])
        np.testing.assert_array_equal(nc, w.want("deep"))
        assert cells == w.cells
        raw, packed = ix.compress_index()
        assert raw >= 1 << 20                                              # (there are cold rows)
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.words)
            nc, cells = node_cover(ix, w.nodes["deep"], tab.p)             # (unpacks)
            np.testing.assert_array_equal(nc, w.want("deep"))
            ix.compress_index()
            nc, cells = node_cover(ix, w.nodes["single"], tab.p)
            np.testing.assert_array_equal(nc, w.want("single"))
    finally:
        ix.close()


def test_everything_is_by_local_genome(hip, wanted):
    """genome_id_base 1000: the intervals are of local genomes, whatever ids the context reports"""
    w = wanted(8)
    ix = w.s.a.build(hip, genome_id_base=1000)
    try:
        nc, cells = ix.taxon_cover(w.s.queries, w.nodes["deep"])
        np.testing.assert_array_equal(nc, w.want("deep"))
        assert cells == w.cells
    finally:
        ix.close()


def test_a_stale_taxonomy_is_refused(hip, wanted):
    w = wanted(8)
    n_g = 200
    ix = w.s.a.build(hip, 0, n_g + 1)
    try:
        lib = ix._lib
        nodes = [(0, n_g + 1), (4, 6)]
        nc, cells = np.full((2, 2), 7, np.uint64), C.c_uint64(7)
        with DevBuf(ix, w.nbytes) as tab, Tax(ix, nodes) as t:
            tab.upload(w.words)
            check(lib.mk_taxonomy_cover(ix._h, t, tab.p, nc.ctypes.data, C.byref(cells)))
            np.testing.assert_array_equal(nc, tcr.node_cover(w.o, w.seen, w.fps, nodes))
            nc[:], cells.value = 7, 7
            ix.select(np.arange(n_g))                                      # the last genome goes: the taxonomy names what was there before
            assert lib.mk_taxonomy_cover(ix._h, t, tab.p, nc.ctypes.data, C.byref(cells)) == MK_ERR_STATE
            assert b"taxonomy" in lib.mk_last_error()
            assert (nc == 7).all() and cells.value == 7
    finally:
        ix.close()


@pytest.mark.parametrize("switch,value", [("MIEKKI_TAXCOVER_ROWS", "0"), ("MIEKKI_TAXCOVER_ROWS", "many"), ("MIEKKI_TAXCOVER_WIDE", "1"),
                                          ("MIEKKI_TAXCOVER_WIDE", "-3"), ("MIEKKI_TAXCOVER_WIDE", "64x")])
def test_a_bad_switch_is_refused(indexes, monkeypatch, switch, value):
    w, ix = indexes(8)
    lib, nodes = ix._lib, w.nodes["deep"]
    monkeypatch.setenv(switch, value)
    nc, cells = np.full((len(nodes), 2), 7, np.uint64), C.c_uint64(7)
    lo = np.array([n[0] for n in nodes], np.uint32)
    hi = np.array([n[1] for n in nodes], np.uint32)
    ptrs, lens = (C.c_char_p * 2)(*w.s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in w.s.queries[:2]])
    with DevBuf(ix, w.nbytes) as tab, Tax(ix, nodes) as t:
        tab.upload(w.words)
        assert lib.mk_taxonomy_cover(ix._h, t, tab.p, nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
        assert switch.encode() in lib.mk_last_error()
        assert lib.mk_query_taxonomy_cover(ix._h, ptrs, lens, 2, lo.ctypes.data, hi.ctypes.data, len(nodes), nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
        assert switch.encode() in lib.mk_last_error()
    assert (nc == 7).all() and cells.value == 7


def test_refusals_leave_the_outputs_alone(hip, indexes):
    w, ix = indexes(8)
    lib, nodes = ix._lib, w.nodes["deep"]
    nc, cells = np.full((len(nodes), 2), 7, np.uint64), C.c_uint64(7)
    lo = np.array([n[0] for n in nodes], np.uint32)
    hi = np.array([n[1] for n in nodes], np.uint32)
    ptrs, lens = (C.c_char_p * 2)(*w.s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in w.s.queries[:2]])
    other = hip.Miekki(*w.s.par)
    try:
        with DevBuf(ix, w.nbytes) as tab, Tax(ix, nodes) as t:
            tab.upload(w.words)
            assert lib.mk_taxonomy_cover(None, t, tab.p, nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            assert b"null argument" in lib.mk_last_error()
            assert lib.mk_taxonomy_cover(ix._h, None, tab.p, nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            assert b"null argument" in lib.mk_last_error()
            assert lib.mk_taxonomy_cover(ix._h, t, tab.p, None, C.byref(cells)) == MK_ERR_ARG
            assert b"null argument" in lib.mk_last_error()
            assert lib.mk_taxonomy_cover(other._h, t, tab.p, nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            assert b"another context" in lib.mk_last_error()
            a = (lo.ctypes.data, hi.ctypes.data, len(nodes))
            assert lib.mk_query_taxonomy_cover(None, ptrs, lens, 2, *a, nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            assert lib.mk_query_taxonomy_cover(ix._h, None, None, 2, *a, nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            assert lib.mk_query_taxonomy_cover(ix._h, ptrs, lens, 2, None, hi.ctypes.data, len(nodes), nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            assert lib.mk_query_taxonomy_cover(ix._h, ptrs, lens, 2, *a, None, C.byref(cells)) == MK_ERR_ARG
            swapped = (hi.ctypes.data, lo.ctypes.data, len(nodes))         # empty intervals: the taxonomy's own refusal
            assert lib.mk_query_taxonomy_cover(ix._h, ptrs, lens, 2, *swapped, nc.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            check(lib.mk_sync(ix._h))
            assert (nc == 7).all() and cells.value == 7
            # cells may be NULL
            check(lib.mk_taxonomy_cover(ix._h, t, tab.p, nc.ctypes.data, None))
            np.testing.assert_array_equal(nc, w.want("deep"))
    finally:
        other.close()


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        nc, cells = ix.taxon_cover(reads, [])
        assert nc.shape == (0, 2) and cells == 0
        lib = ix._lib
        marks = np.arange(7, 11, dtype=np.uint64)
        out, n = marks.copy(), C.c_uint64(99)
        ptrs, lens = (C.c_char_p * 2)(*reads), (C.c_uint64 * 2)(*[len(r) for r in reads])
        assert lib.mk_query_taxonomy_cover(ix._h, ptrs, lens, 2, None, None, 0, out.ctypes.data, C.byref(n)) == MK_OK
        assert n.value == 0
        assert lib.mk_query_taxonomy_cover(ix._h, ptrs, lens, 2, None, None, 0, None, None) == MK_OK
        table = np.arange(4096, dtype=np.uint32)
        with DevBuf(ix, 16384) as tab, Tax(ix, []) as t:
            tab.upload(table)
            n = C.c_uint64(99)
            assert lib.mk_taxonomy_cover(ix._h, t, tab.p, None, C.byref(n)) == MK_OK
            assert n.value == int(np.unpackbits(table.view(np.uint8)).sum())     # a taxonomy without nodes: the table's cells
            assert lib.mk_taxonomy_cover(ix._h, t, tab.p, out.ctypes.data, None) == MK_OK
            assert lib.mk_taxonomy_cover(ix._h, t, None, out.ctypes.data, C.byref(n)) == MK_OK and n.value == 0
        np.testing.assert_array_equal(out, marks)                          # out is not written
    finally:
        ix.close()
