"""mk_cover_assign / mk_cover_winners / mk_query_cover_winners and Miekki.cover_winners: the winner-takes-all screen -- every seen
cell credited to the best-ranked genome that holds it -- must be, count for count, what tests/winners_ref.py makes of the
ORACLE's gated sketches and stored columns: P = 512, G = 1,101 at one byte and 603 at two, two 1 KiB tiles per row with a ragged
second one."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import cover_ref as cr
import synth
import winners_ref as wr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MK_OK, MK_ERR_ARG = 0, -1
WIDTHS = [8, 16]
ROWS = [1, 7, 512]


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


@pytest.fixture(scope="module")
def samples():
    return wr.samples()


@pytest.fixture(scope="module")
def indexes(hip, samples):
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = samples(bits).s.a.build(hip)
        return samples(bits), made[bits]
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


def winners(ix, tab):
    """mk_cover_winners: (covered, won, cells, claimed)"""
    G = ix.index_size
    cov, won = np.full(G, 0xdead, np.uint32), np.full(G, 0xdead, np.uint32)
    cells, claimed = C.c_uint64(0xdead), C.c_uint64(0xdead)
    check(ix._lib.mk_cover_winners(ix._h, tab.p, cov.ctypes.data, won.ctypes.data, C.byref(cells), C.byref(claimed)))
    return cov, won, int(cells.value), int(claimed.value)


def assign(ix, tab, order):
    """mk_cover_assign: (won, claimed)"""
    order = np.ascontiguousarray(order, np.uint32)
    won, claimed = np.full(ix.index_size, 0xdead, np.uint32), C.c_uint64(0xdead)
    check(ix._lib.mk_cover_assign(ix._h, tab.p, order.ctypes.data, won.ctypes.data, C.byref(claimed)))
    return won, int(claimed.value)


def same(got, w, cov, won, cells, claimed):
    np.testing.assert_array_equal(got[0], cov)
    np.testing.assert_array_equal(got[1], won)
    assert got[2:] == (cells, claimed)


@pytest.mark.parametrize("bits", WIDTHS)
def test_full_sample_like_the_yardstick(indexes, bits):
    """through the pieces (a table marked by mk_qset_run_cover, mk_cover_winners) and in one call (Miekki.cover_winners =
    mk_query_cover_winners); the win pass is carried by filter_ms"""
    w, ix = indexes(bits)
    with Table(ix, w.s.queries) as tab:
        ix.reset_stats()
        got = winners(ix, tab)
        assert ix.stats()["filter_ms"] > 0
        same(got, w, w.cov, w.won, w.cells, w.claimed)
        won, claimed = assign(ix, tab, w.order)                            # the yardstick's order, handed in
        np.testing.assert_array_equal(won, w.won)
        assert claimed == w.claimed
    got = ix.cover_winners(w.s.queries)
    assert got[0].dtype == got[1].dtype == np.uint32 and got[1].shape == (w.G,)
    same(got, w, w.cov, w.won, w.cells, w.claimed)
    assert got[1].sum() == got[3] and (got[1] <= got[0]).all() and got[1][w.order[0]] == got[0][w.order[0]]


@pytest.mark.parametrize("bits", WIDTHS)
def test_results_do_not_depend_on_how_the_reads_are_split(indexes, bits):
    w, ix = indexes(bits)
    q = w.s.queries
    with Table(ix, q[:300], q[300:]) as tab:                               # halves
        same(winners(ix, tab), w, w.cov, w.won, w.cells, w.claimed)
    with Table(ix, q, q) as tab:                                           # the set twice
        same(winners(ix, tab), w, w.cov, w.won, w.cells, w.claimed)
    seen, cov, order, won, claimed = w.of(q[:40])                          # the first 40 reads only
    assert 0 < claimed < w.claimed
    same(ix.cover_winners(q[:40]), w, cov, won, int(seen.sum()), claimed)


@pytest.mark.parametrize("bits", WIDTHS)
def test_caller_given_orders(indexes, bits):
    """the reverse of the natural order, and a seeded random permutation, against the yardstick with the same order"""
    w, ix = indexes(bits)
    with Table(ix, w.s.queries) as tab:
        for order in (np.arange(w.G)[::-1], np.random.default_rng(77).permutation(w.G)):
            want, claimed = wr.won(w.o, w.seen, w.fps, order)
            assert (want != w.won).any()
            got, n = assign(ix, tab, order)
            np.testing.assert_array_equal(got, want)
            assert n == claimed == w.claimed                               # who wins changes, what is held does not
            assert got[order[0]] == w.cov[order[0]]


@pytest.mark.parametrize("bits", WIDTHS)
def test_uploaded_tables_all_ones_and_all_zero(indexes, bits):
    """every bit set: every live stored fingerprint competes, the bit of `empty` counts for nothing, the rows' zero padding
    claims nothing -- claimed is the number of distinct (p, v != empty) of the matrix; no bit set: nothing is won"""
    w, ix = indexes(bits)
    o = w.o
    ones = np.ones((w.P, 1 << bits), bool)
    live = w.fps != cr.empty_of(o)
    held = np.zeros((w.P, 1 << bits), bool)
    held[np.nonzero(live)[0], w.fps[live]] = True
    assert held[:, 0].sum() < w.P                                          # some row holds no 0: its padding must not claim (p, 0)
    cov = cr.covered(o, ones, w.fps)
    np.testing.assert_array_equal(cov, o.sketch_size)
    order = wr.order(cov, o.sketch_size)
    won, claimed = wr.won(o, ones, w.fps, order)
    assert claimed == held.sum()
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(np.full(w.nbytes // 4, 0xffffffff, np.uint32))
        same(winners(ix, tab), w, cov, won, w.P << bits, claimed)
        tab.upload(np.zeros(w.nbytes // 4, np.uint32))
        got = winners(ix, tab)
        assert not got[0].any() and not got[1].any() and got[2:] == (0, 0)
        only_empty = np.zeros((w.P, 1 << bits), bool)
        only_empty[:, cr.empty_of(o)] = True
        tab.upload(cr.pack(only_empty))
        got = winners(ix, tab)
        assert not got[1].any() and got[2:] == (w.P, 0)


@pytest.fixture(scope="module")
def chunked(samples, tmp_path_factory):
    """mk_cover_winners over the yardstick's table in fresh processes (tests/winners_worker.py), one per width and
    MIEKKI_WIN_ROWS, all at once"""
    d = tmp_path_factory.mktemp("winners_rows")
    procs = {}
    for bits in WIDTHS:
        w = samples(bits)
        with open(d / f"job_{bits}.pkl", "wb") as f:
            pickle.dump({"par": w.s.c.par, "seqs": w.s.c.seqs, "words": w.words}, f)
        for rows in ROWS:
            env = dict(os.environ, MIEKKI_WIN_ROWS=str(rows))
            env.pop("MIEKKI_WIN_VALUES", None)
            procs[bits, rows] = subprocess.Popen([sys.executable, os.path.join(HERE, "winners_worker.py"), str(d / f"job_{bits}.pkl"),
                                                  str(d / f"out_{bits}_{rows}.npz")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for (bits, rows), p in procs.items():
        text = p.communicate(timeout=300)[0]
        assert p.returncode == 0, text.decode(errors="replace")[-3000:]
        out[bits, rows] = dict(np.load(d / f"out_{bits}_{rows}.npz"))
    return out


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("bits", WIDTHS)
def test_row_chunks_give_identical_results(samples, chunked, bits, rows):
    w, got = samples(bits), chunked[bits, rows]
    same((got["covered"], got["won"], int(got["cells"]), int(got["claimed"])), w, w.cov, w.won, w.cells, w.claimed)


@pytest.mark.parametrize("switch", [None, "MIEKKI_WIN_TOUCHED", "MIEKKI_WIN_FILTER"])
@pytest.mark.parametrize("values", ["256", "4096", None, "32768"])
def test_value_ranges_at_two_bytes(indexes, monkeypatch, values, switch):
    """256 ranges of 256 values, 16 of 4,096, the default, the largest that fits -- with the touched slots listed, with the
    whole range read out (MIEKKI_WIN_TOUCHED=0), and without the plain read in front of the atomic (MIEKKI_WIN_FILTER=0)"""
    w, ix = indexes(16)
    if values:
        monkeypatch.setenv("MIEKKI_WIN_VALUES", values)
    if switch:
        monkeypatch.setenv(switch, "0")
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(w.words)
        same(winners(ix, tab), w, w.cov, w.won, w.cells, w.claimed)


@pytest.mark.parametrize("values", ["65536", "3000", "128"])
def test_a_range_that_does_not_fit_is_refused(indexes, monkeypatch, values):
    w, ix = indexes(16)
    monkeypatch.setenv("MIEKKI_WIN_VALUES", values)
    lib = ix._lib
    cov, won = np.full(w.G, 7, np.uint32), np.full(w.G, 7, np.uint32)
    cells, claimed = C.c_uint64(7), C.c_uint64(7)
    order = np.arange(w.G, dtype=np.uint32)
    ptrs, lens = (C.c_char_p * 2)(*w.s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in w.s.queries[:2]])
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(w.words)
        assert lib.mk_cover_assign(ix._h, tab.p, order.ctypes.data, won.ctypes.data, C.byref(claimed)) == MK_ERR_ARG
        assert b"MIEKKI_WIN_VALUES" in lib.mk_last_error()
        assert lib.mk_cover_winners(ix._h, tab.p, cov.ctypes.data, won.ctypes.data, C.byref(cells), C.byref(claimed)) == MK_ERR_ARG
        assert lib.mk_query_cover_winners(ix._h, ptrs, lens, 2, cov.ctypes.data, won.ctypes.data, C.byref(cells), C.byref(claimed)) == MK_ERR_ARG
    assert (cov == 7).all() and (won == 7).all() and cells.value == claimed.value == 7
    # one byte has one range of 256: the switch is not read -- and the answer is the same without the filter
    monkeypatch.setenv("MIEKKI_WIN_FILTER", "0")
    w8, ix8 = indexes(8)
    with DevBuf(ix8, w8.nbytes) as tab:
        tab.upload(w8.words)
        same(winners(ix8, tab), w8, w8.cov, w8.won, w8.cells, w8.claimed)


def test_more_touched_slots_than_the_list_holds(hip, monkeypatch):
    """10,000 unrelated genomes at two bytes, an all-ones table and ranges of 32,768 values: more values of a row fall into a
    range than the 2,048 the list of touched slots holds, so the whole range is read out.  No oracle at this size: the index's
    own exported columns, ranked and dealt out in numpy, and MIEKKI_WIN_TOUCHED=0."""
    G, P, bits = 10_000, 512, 16
    ix = hip.Miekki(15, 9, bits, 32, 20)
    try:
        ix.insert_synthetic(0, G, 3000)
        cols = np.empty(P * G * 2, np.uint8)
        check(ix._lib.mk_index_export_columns(ix._h, 0, P, cols.ctypes.data))
        fps = cols.view(np.uint16).reshape(P, G).astype(np.int64)          # (either byte order: 0xffff is `empty` in both)
        live = fps != 0xffff
        ss = ix.sketch_size
        np.testing.assert_array_equal(live.sum(0), ss)
        order = wr.order(ss, ss)                                           # all ones: covered = sketch_size
        rank = wr.rank_of(order)
        p, g = np.nonzero(live)
        cell = (p.astype(np.int64) << bits) + fps[p, g]
        at = np.lexsort((rank[g], cell))
        cell, g = cell[at], g[at]
        first = np.ones(len(cell), bool)
        first[1:] = cell[1:] != cell[:-1]
        want = np.bincount(g[first], minlength=G).astype(np.uint32)
        per_range = np.bincount(cell[first] >> 15)                         # claimed cells per (row, range of 32,768)
        assert per_range.min() > 2048 and (want != ss).any()
        monkeypatch.setenv("MIEKKI_WIN_VALUES", "32768")
        nbytes = (P << bits) >> 3
        with DevBuf(ix, nbytes) as tab:
            tab.upload(np.full(nbytes // 4, 0xffffffff, np.uint32))
            got = winners(ix, tab)
            np.testing.assert_array_equal(got[0], ss)
            np.testing.assert_array_equal(got[1], want)
            assert got[2:] == (P << bits, int(first.sum()))
            monkeypatch.setenv("MIEKKI_WIN_TOUCHED", "0")
            np.testing.assert_array_equal(winners(ix, tab)[1], want)
    finally:
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_cold_rows_raw_and_packed(hip, samples, monkeypatch, bits):
    """1 MiB of a 2 MiB matrix in HBM (a reservation doubles the rows' pitch), the other rows in host memory: read where they
    lie; then packed (compress_index), which the passes unpack first"""
    w = samples(bits)
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = hip.Miekki(*w.s.c.par)
    try:
        ix.reserve(4096 * 8 // bits)
        for i in range(0, w.G, 64):
            ix.insert_sequences(w.s.c.seqs[i:i + 64])
        same(ix.cover_winners(w.s.queries), w, w.cov, w.won, w.cells, w.claimed)
        raw, packed = ix.compress_index()
        assert raw >= 1 << 20                                              # (there are cold rows)
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.words)
            won, claimed = assign(ix, tab, w.order)                        # (unpacks)
            np.testing.assert_array_equal(won, w.won)
            assert claimed == w.claimed
            ix.compress_index()
            same(winners(ix, tab), w, w.cov, w.won, w.cells, w.claimed)
    finally:
        ix.close()


def test_everything_is_by_local_genome(hip, samples):
    """genome_id_base 1000: order, covered and won are by local genome, whatever ids the context reports"""
    w = samples(8)
    ix = w.s.a.build(hip, genome_id_base=1000)
    try:
        same(ix.cover_winners(w.s.queries), w, w.cov, w.won, w.cells, w.claimed)
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.words)
            same(winners(ix, tab), w, w.cov, w.won, w.cells, w.claimed)
            order = np.arange(w.G)[::-1]
            np.testing.assert_array_equal(assign(ix, tab, order)[0], wr.won(w.o, w.seen, w.fps, order)[0])
            bad = (order + 1000).astype(np.uint32)                         # the context's ids are not what an order names
            won, claimed = np.full(w.G, 7, np.uint32), C.c_uint64(7)
            assert ix._lib.mk_cover_assign(ix._h, tab.p, bad.ctypes.data, won.ctypes.data, C.byref(claimed)) == MK_ERR_ARG
            assert (won == 7).all() and claimed.value == 7
    finally:
        ix.close()


def test_refusals_leave_the_outputs_alone(indexes):
    w, ix = indexes(8)
    lib, G = ix._lib, w.G
    cov, won = np.full(G, 7, np.uint32), np.full(G, 7, np.uint32)
    cells, claimed = C.c_uint64(7), C.c_uint64(7)
    order = np.arange(G, dtype=np.uint32)
    repeated, beyond = order.copy(), order.copy()
    repeated[G - 1] = 5
    beyond[17] = G
    ptrs, lens = (C.c_char_p * 2)(*w.s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in w.s.queries[:2]])
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(w.words)
        a = (order.ctypes.data, won.ctypes.data, C.byref(claimed))
        assert lib.mk_cover_assign(None, tab.p, *a) == MK_ERR_ARG
        assert lib.mk_cover_assign(ix._h, None, *a) == MK_ERR_ARG
        assert lib.mk_cover_assign(ix._h, tab.p, None, won.ctypes.data, C.byref(claimed)) == MK_ERR_ARG
        assert lib.mk_cover_assign(ix._h, tab.p, order.ctypes.data, None, C.byref(claimed)) == MK_ERR_ARG
        assert lib.mk_cover_assign(ix._h, tab.p, repeated.ctypes.data, won.ctypes.data, C.byref(claimed)) == MK_ERR_ARG
        assert b"permutation" in lib.mk_last_error()
        assert lib.mk_cover_assign(ix._h, tab.p, beyond.ctypes.data, won.ctypes.data, C.byref(claimed)) == MK_ERR_ARG
        b = (C.byref(cells), C.byref(claimed))
        assert lib.mk_cover_winners(None, tab.p, cov.ctypes.data, won.ctypes.data, *b) == MK_ERR_ARG
        assert lib.mk_cover_winners(ix._h, None, cov.ctypes.data, won.ctypes.data, *b) == MK_ERR_ARG
        assert lib.mk_cover_winners(ix._h, tab.p, None, won.ctypes.data, *b) == MK_ERR_ARG
        assert lib.mk_cover_winners(ix._h, tab.p, cov.ctypes.data, None, *b) == MK_ERR_ARG
        assert lib.mk_query_cover_winners(ix._h, None, None, 3, cov.ctypes.data, won.ctypes.data, *b) == MK_ERR_ARG
        assert lib.mk_query_cover_winners(ix._h, ptrs, lens, 2, None, won.ctypes.data, *b) == MK_ERR_ARG
        assert lib.mk_query_cover_winners(ix._h, ptrs, lens, 2, cov.ctypes.data, None, *b) == MK_ERR_ARG
        check(lib.mk_sync(ix._h))
        assert (cov == 7).all() and (won == 7).all() and cells.value == claimed.value == 7
        # cells and claimed may be NULL
        check(lib.mk_cover_winners(ix._h, tab.p, cov.ctypes.data, won.ctypes.data, None, None))
        np.testing.assert_array_equal(cov, w.cov)
        np.testing.assert_array_equal(won, w.won)
        given = w.order.astype(np.uint32)
        check(lib.mk_cover_assign(ix._h, tab.p, given.ctypes.data, won.ctypes.data, None))
        np.testing.assert_array_equal(won, w.won)


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        cov, won, cells, claimed = ix.cover_winners(reads)
        assert cov.shape == won.shape == (0,) and cells == claimed == 0
        lib = ix._lib
        marks = np.arange(7, 11, dtype=np.uint32)
        cov, won = marks.copy(), marks.copy()
        n, m = C.c_uint64(99), C.c_uint64(99)
        ptrs, lens = (C.c_char_p * 2)(*reads), (C.c_uint64 * 2)(*[len(r) for r in reads])
        assert lib.mk_query_cover_winners(ix._h, ptrs, lens, 2, cov.ctypes.data, won.ctypes.data, C.byref(n), C.byref(m)) == MK_OK
        assert n.value == m.value == 0
        assert lib.mk_query_cover_winners(ix._h, ptrs, lens, 2, None, None, None, None) == MK_OK
        table = np.arange(4096, dtype=np.uint32)
        with DevBuf(ix, 16384) as tab:
            tab.upload(table)
            n, m = C.c_uint64(99), C.c_uint64(99)
            assert lib.mk_cover_assign(ix._h, tab.p, None, None, C.byref(m)) == MK_OK and m.value == 0
            assert lib.mk_cover_assign(ix._h, tab.p, marks.ctypes.data, won.ctypes.data, None) == MK_OK
            m = C.c_uint64(99)
            assert lib.mk_cover_winners(ix._h, tab.p, None, None, C.byref(n), C.byref(m)) == MK_OK
            assert m.value == 0 and n.value == int(np.unpackbits(table.view(np.uint8)).sum())
        np.testing.assert_array_equal(cov, marks)                          # covered and won are not written
        np.testing.assert_array_equal(won, marks)
    finally:
        ix.close()
