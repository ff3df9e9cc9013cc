"""mk_panel_bytes / mk_panel_reset / mk_qset_run_panel / mk_panel_count / mk_panel_slot / mk_query_panel and Miekki.panel: the
cover of up to eight samples from one table of bytes -- bit s of a cell's byte: sample s has seen it -- and ONE pass over the
matrix must be, byte for byte and count for count, what tests/panel_ref.py makes of the ORACLE's gated sketches and stored
columns sample by sample; and, with no oracle, what the cover that exists (mk_qset_run_cover, mk_cover_count) gives per sample."""
import ctypes as C

import numpy as np
import pytest

import cover_ref as cr
import panel_ref as pr
import synth
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_STATE = 0, -1, -5
WIDTHS = [8, 16]
MARK = 0xdeadbeef


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """a tr.Sample dealt into eight samples, with the oracle's table and counts of them, each computed once"""

    def __init__(self, *args, **kw):
        self.s = s = tr.Sample(*args, **kw)
        self.o = o = s.o
        self.h, self.bits, self.P, self.G = o.number_minimizer_log2, o.number_bit_minimizer, o.P, o.index_size
        self.fps = cr.stored(o)
        self.dealt = pr.deal(s)
        self.seens = pr.seen_per_sample(o, self.dealt)
        self.tab = pr.table(self.seens)
        self.cov, self.cells = pr.covered(o, self.seens, self.fps), pr.cells(self.seens)
        self.nbytes = self.P << self.bits

    def count(self, tab, n_slots=8):
        return pr.count_table(self.o, tab, n_slots, self.fps)


@pytest.fixture(scope="module")
def samples():
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Wanted() if bits == 8 else Wanted(603, 16, 320_000, whole=())
        return made[bits]
    return get


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

    def upload(self, arr, at=0):
        check(self.ix._lib.mk_dev_upload(self.ix._h, C.c_void_p(self.p.value + at), arr.ctypes.data, arr.nbytes))

    def download(self):
        arr = np.zeros(self.nbytes, np.uint8)
        check(self.ix._lib.mk_dev_download(self.ix._h, arr.ctypes.data, self.p, arr.nbytes))
        return arr


class Table(DevBuf):
    """a panel table of the index's own size, reset"""

    def __init__(self, ix):
        n = ix._lib.mk_panel_bytes(ix._h)
        assert n == 1 << ix._p.h << ix._p.fp_bits == ix._lib.mk_depth_bytes(ix._h)
        DevBuf.__init__(self, ix, n)
        check(ix._lib.mk_panel_reset(ix._h, self.p))


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


def run(ix, qs, slot, tab):
    return ix._lib.mk_qset_run_panel(ix._h, qs, slot, tab.p)


def mark(ix, seqs, slot, tab):
    with Uploaded(ix, seqs) as qs:
        check(run(ix, qs, slot, tab))


def count(ix, tab, n_slots=8, G=None):
    """mk_panel_count: (covered [n_slots, G], cells [n_slots]); the room behind both outputs is untouched"""
    G = ix.index_size if G is None else G
    cov = np.full((n_slots + 1) * G + 1, MARK, np.uint32)
    cells = np.full(n_slots + 1, MARK, np.uint64)
    check(ix._lib.mk_panel_count(ix._h, tab.p, n_slots, cov.ctypes.data, cells.ctypes.data))
    assert (cov[n_slots * G:] == MARK).all() and cells[n_slots] == MARK
    return cov[:n_slots * G].reshape(n_slots, G).copy(), cells[:n_slots].copy()


def same(got, want):
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("filt", [None, "0"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_marks_are_the_reference_table(indexes, monkeypatch, bits, filt):
    """the downloaded table, byte for byte: every sample in one pass into its slot; after a reset one sample in two halves, one
    marked twice, the slots in another order -- with the plain load in front of the atomic and without it; no scan is launched"""
    w, ix = indexes(bits)
    if filt:
        monkeypatch.setenv("MIEKKI_PANEL_FILTER", filt)
    ix.reset_stats()
    before = ix.stats()["scan_launches"]
    with Table(ix) as tab:
        assert tab.nbytes == w.nbytes
        for slot, q in enumerate(w.dealt):
            mark(ix, q, slot, tab)
        np.testing.assert_array_equal(tab.download(), w.tab)
        same(count(ix, tab), (w.cov, w.cells))
        check(ix._lib.mk_panel_reset(ix._h, tab.p))
        assert not tab.download().any()
        for slot in (7, 3, 5, 0, 1, 2, 6):
            mark(ix, w.dealt[slot], slot, tab)
        half = len(w.dealt[4]) // 2
        mark(ix, w.dealt[4][:half], 4, tab)                                  # in two halves
        mark(ix, w.dealt[4][half:], 4, tab)
        with Uploaded(ix, w.dealt[0]) as qs:                                 # twice: an OR
            check(run(ix, qs, 0, tab))
            check(run(ix, qs, 0, tab))
        np.testing.assert_array_equal(tab.download(), w.tab)
    st = ix.stats()
    assert st["scan_launches"] == before and st["sketch_ms"] > 0 and st["filter_ms"] > 0


@pytest.mark.parametrize("rows", [None, "1", "24", "44"])
@pytest.mark.parametrize("n_slots", [1, 3, 8])
@pytest.mark.parametrize("bits", WIDTHS)
def test_counts_like_the_oracle(indexes, monkeypatch, bits, n_slots, rows):
    """the yardstick's table of all eight samples counted for 1, 3 and 8 slots -- the others are marked and not reported, the
    room behind the outputs stays as it was -- in the default chunks of rows, in chunks of one row, of 24 (no whole stage of 32
    rows at 8 bits) and of 44 (a stage, then a partial one of 12 rows: groups of four)"""
    w, ix = indexes(bits)
    if rows:
        monkeypatch.setenv("MIEKKI_PANEL_ROWS", rows)
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(w.tab)
        same(count(ix, tab, n_slots), (w.cov[:n_slots], w.cells[:n_slots]))


@pytest.mark.parametrize("rows", [None, "42"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_uploaded_tables_alone(indexes, monkeypatch, bits, rows):
    """chunks of 42 rows end in a partial group of two"""
    w, ix = indexes(bits)
    if rows:
        monkeypatch.setenv("MIEKKI_PANEL_ROWS", rows)
    ss = w.o.sketch_size
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(np.full(w.nbytes, 255, np.uint8))                        # all 32 counters of a word carry at once
        cov, cells = count(ix, tab)
        np.testing.assert_array_equal(cov, np.tile(ss, (8, 1)))
        assert (cells == w.P << bits).all()
        only_empty = np.zeros((w.P, 1 << bits), np.uint8)
        only_empty[:, cr.empty_of(w.o)] = 255
        tab.upload(only_empty.reshape(-1))                                  # a genome without a fingerprint never counts
        cov, cells = count(ix, tab)
        assert not cov.any() and (cells == w.P).all()
        zero_only = np.zeros((w.P, 1 << bits), np.uint8)
        zero_only[:, 0] = 0xa5                                              # value 0 everywhere: the rows' zero padding is not genomes
        tab.upload(zero_only.reshape(-1))
        cov, cells = count(ix, tab)
        at0 = (w.fps == 0).sum(0).astype(np.uint32)
        on = np.array([(0xa5 >> s) & 1 for s in range(8)], np.uint32)
        np.testing.assert_array_equal(cov, on[:, None] * at0[None, :])
        np.testing.assert_array_equal(cells, on.astype(np.uint64) * w.P)
        noise = np.random.default_rng(3).integers(0, 256, w.nbytes, dtype=np.uint8)
        live = w.fps != cr.empty_of(w.o)
        cells_at = noise.reshape(w.P, -1)[np.arange(w.P)[:, None], w.fps]
        want = np.stack([(((cells_at >> s) & 1) & live).sum(0) for s in range(8)]).astype(np.uint32)
        tab.upload(noise)                                                   # no slot bleeds into another, no genome into its neighbour
        cov, cells = count(ix, tab)
        np.testing.assert_array_equal(cov, want)
        np.testing.assert_array_equal(cells, [int(((noise >> s) & 1).sum()) for s in range(8)])
        assert len({c.tobytes() for c in want}) == 8
        same((cov, cells), w.count(noise))


class Large:
    """40 genomes of 200 kb at -h 17 (8 bits) and -h 15 (16 bits): more than twice the rows any chunk may have, and sketch
    sizes beyond what a counter of the bit planes holds.  The oracle's sketch sizes and the index, once per width."""

    K, N, LEN = 31, 40, 200_000

    def __init__(self, hip, bits):
        from oracle import oracle as orc
        self.H = 17 if bits == 8 else 15
        self.seqs = [synth.genome_bases(7_000_000 + g, 0, self.LEN) for g in range(self.N)]
        self.o = orc.OracleMiekki(self.K, self.H, bits, 32, 200)
        self.o.insert_sequences(self.seqs)
        self.ix = hip.Miekki(self.K, self.H, bits, 32, 200)
        self.ix.insert_sequences(self.seqs)


@pytest.fixture(scope="module")
def large(hip):
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Large(hip, bits)
        return made[bits]
    yield get
    for l in made.values():
        l.ix.close()


@pytest.mark.parametrize("rows", [None, "1048576"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_counts_reach_the_sketch_size_beyond_the_planes(large, monkeypatch, bits, rows):
    """an all-0xFF table counts to the sketch size, above 16,383, in every slot -- in the default chunks and with a chunk asked
    for that is larger than the index, which the host clamps to what a counter holds"""
    l = large(bits)
    ix, ss = l.ix, l.o.sketch_size
    assert ss.min() > 16_383 and (1 << l.H) > 2 * 16_383
    if rows:
        monkeypatch.setenv("MIEKKI_PANEL_ROWS", rows)
    nbytes = 1 << l.H << bits
    full = np.full(min(nbytes, 16 << 20), 255, np.uint8)
    with DevBuf(ix, nbytes) as tab:
        for at in range(0, nbytes, full.nbytes):
            tab.upload(full, at)
        cov, cells = count(ix, tab)
    np.testing.assert_array_equal(cov, np.tile(ss, (8, 1)))
    assert (cells == nbytes).all()


@pytest.mark.parametrize("bits,H", [(8, 14), (16, 11)])
def test_agreement_with_the_cover_that_exists(hip, bits, H):
    """no oracle: strain reads dealt into eight samples (-h 14 at 8 bits; -h 11 at 16, where the tables are eight times those of
    -h 14 at 8).  mk_panel_slot of each slot is bit for bit the table mk_qset_run_cover makes of that sample, and mk_cover_count
    of the extracted table is that slot's row and cell count of mk_panel_count"""
    SP, ST, SL, PPM = 3, 48, 50_000, 3000
    G = SP * ST
    seqs = [synth.strain_device(g, ST, PPM, 0, SL) for g in range(G)]
    ix = hip.Miekki(31, H, bits, 33, 200)
    lib = ix._lib
    try:
        for g0 in range(0, G, 48):
            ix.insert_sequences(seqs[g0:g0 + 48])
        rng = np.random.default_rng(11)
        reads = []
        for _ in range(300):
            g = int(rng.integers(0, G))
            off = int(rng.integers(0, SL - 1000))
            reads.append(seqs[g][off:off + 1000])
        cuts = [0, 90, 91, 91, 140, 200, 230, 290, 300]
        dealt = [reads[cuts[i]:cuts[i + 1]] for i in range(8)]
        nseen = lib.mk_cover_bytes(ix._h)
        with Table(ix) as tab, DevBuf(ix, nseen) as plane, DevBuf(ix, nseen) as seen:
            for slot, q in enumerate(dealt):
                mark(ix, q, slot, tab)
            cov, cells = count(ix, tab)
            assert cov.max() > 400 and not cov[2].any() and cells[2] == 0
            for slot, q in enumerate(dealt):
                plane.upload(np.full(nseen, 0x5a, np.uint8))                 # (written, not OR-ed into)
                check(lib.mk_panel_slot(ix._h, tab.p, slot, plane.p))
                check(lib.mk_cover_reset(ix._h, seen.p))
                with Uploaded(ix, q) as qs:
                    check(lib.mk_qset_run_cover(ix._h, qs, seen.p))
                check(lib.mk_sync(ix._h))
                np.testing.assert_array_equal(plane.download(), seen.download())
                cov1, cells1 = np.zeros(G, np.uint32), C.c_uint64(0)
                check(lib.mk_cover_count(ix._h, plane.p, cov1.ctypes.data, C.byref(cells1)))
                np.testing.assert_array_equal(cov[slot], cov1)
                assert int(cells[slot]) == cells1.value
    finally:
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_cold_rows_raw_and_packed(hip, samples, monkeypatch, bits):
    """1 MiB of a 2 MiB matrix in HBM (a reservation doubles the rows' pitch), the other rows in host memory: read where they
    lie; then packed (compress_index), which the count unpacks first"""
    w = samples(bits)
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = hip.Miekki(*w.s.c.par)
    try:
        ix.reserve(4096 * 8 // bits)
        for i in range(0, w.G, 64):
            ix.insert_sequences(w.s.c.seqs[i:i + 64])
        same(ix.panel(w.dealt), (w.cov, w.cells))
        raw, packed = ix.compress_index()
        assert raw >= 1 << 20                                              # (there are cold rows)
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.tab)
            same(count(ix, tab), (w.cov, w.cells))
        ix.compress_index()
        same(ix.panel(w.dealt[:3]), (w.cov[:3], w.cells[:3]))
    finally:
        ix.close()


def test_results_are_by_local_genome(hip, samples):
    """genome_id_base 1000: covered[s][j] is local genome j's, whatever ids the context reports"""
    w = samples(8)
    ix = w.s.a.build(hip, genome_id_base=1000)
    try:
        same(ix.panel(w.dealt), (w.cov, w.cells))
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.tab)
            same(count(ix, tab, 3), (w.cov[:3], w.cells[:3]))
    finally:
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_python_panel_of_eleven_samples_and_of_none(indexes, bits):
    """8 + 3 samples: two groups through one table, the second after a reset; one of the three is empty"""
    w, ix = indexes(bits)
    more = [w.dealt[0][:5], [], w.dealt[4][:20]]
    seens = pr.seen_per_sample(w.o, more)
    cov, cells = ix.panel(w.dealt + more)
    assert cov.shape == (11, w.G) and cells.shape == (11,)
    same((cov, cells), (np.concatenate([w.cov, pr.covered(w.o, seens, w.fps)]), np.concatenate([w.cells, pr.cells(seens)])))
    assert not cov[9].any() and cov[8].any() and cov[10].any()
    cov, cells = ix.panel([])
    assert cov.shape == (0, w.G) and cells.shape == (0,) and cov.dtype == np.uint32 and cells.dtype == np.uint64


def test_refusals_leave_the_table_and_the_outputs_alone(hip, samples):
    from oracle import oracle as orc
    w = samples(8)
    s, G = w.s, 200
    o = orc.OracleMiekki(*s.c.par)                                          # (the gate is the Bloom filter of these 200 genomes)
    o.insert_sequences(s.c.seqs[:G])
    fps = cr.stored(o)
    ix = s.a.build(hip, 0, G)
    lib = ix._lib
    try:
        marks = np.random.default_rng(3).integers(0, 256, w.nbytes, dtype=np.uint8)
        cov, cells = np.full(8 * G, MARK, np.uint32), np.full(8, MARK, np.uint64)
        nseen = lib.mk_cover_bytes(ix._h)
        with DevBuf(ix, w.nbytes) as tab, DevBuf(ix, nseen) as plane, Uploaded(ix, s.queries[:40]) as qs, Uploaded(ix, []) as none, \
                FromIndex(ix, np.arange(G)) as own:
            tab.upload(marks)
            plane.upload(np.full(nseen, 0x5a, np.uint8))
            assert lib.mk_qset_run_panel(None, qs, 0, tab.p) == MK_ERR_ARG
            assert lib.mk_qset_run_panel(ix._h, None, 0, tab.p) == MK_ERR_ARG
            assert lib.mk_qset_run_panel(ix._h, qs, 0, None) == MK_ERR_ARG
            assert lib.mk_qset_run_panel(ix._h, qs, 8, tab.p) == MK_ERR_ARG
            assert lib.mk_panel_reset(ix._h, None) == MK_ERR_ARG
            assert lib.mk_panel_reset(None, tab.p) == MK_ERR_ARG
            assert lib.mk_panel_count(None, tab.p, 8, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_panel_count(ix._h, None, 8, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_panel_count(ix._h, tab.p, 8, None, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_panel_count(ix._h, tab.p, 0, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_panel_count(ix._h, tab.p, 9, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_panel_slot(None, tab.p, 0, plane.p) == MK_ERR_ARG
            assert lib.mk_panel_slot(ix._h, None, 0, plane.p) == MK_ERR_ARG
            assert lib.mk_panel_slot(ix._h, tab.p, 0, None) == MK_ERR_ARG
            assert lib.mk_panel_slot(ix._h, tab.p, 8, plane.p) == MK_ERR_ARG
            ptrs, lens = (C.c_char_p * 3)(*s.queries[:3]), (C.c_uint64 * 3)(*[len(q) for q in s.queries[:3]])
            starts, falling = (C.c_uint64 * 3)(0, 1, 3), (C.c_uint64 * 3)(0, 2, 1)
            assert lib.mk_query_panel(None, ptrs, lens, starts, 2, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_panel(ix._h, None, lens, starts, 2, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_panel(ix._h, ptrs, None, starts, 2, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_panel(ix._h, ptrs, lens, None, 2, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_panel(ix._h, ptrs, lens, starts, 2, None, cells.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_panel(ix._h, ptrs, lens, falling, 2, cov.ctypes.data, cells.ctypes.data) == MK_ERR_ARG
            assert run(ix, none, 3, tab) == MK_OK                           # an empty set
            ix.select(np.arange(G - 1))                                     # `own` names what was there before
            assert run(ix, own, 3, tab) == MK_ERR_STATE
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(tab.download(), marks)
            assert (plane.download() == 0x5a).all()
            assert (cov == MARK).all() and (cells == MARK).all()
            check(run(ix, qs, 5, tab))                                      # ... and an uploaded set still runs: its bits are OR-ed in
            want = marks | (cr.seen(o, s.queries[:40]).reshape(-1).astype(np.uint8) << np.uint8(5))
            np.testing.assert_array_equal(tab.download(), want)
            got = np.zeros((8, G - 1), np.uint32)
            check(lib.mk_panel_count(ix._h, tab.p, 8, got.ctypes.data, None))   # cells may be NULL
            np.testing.assert_array_equal(got, pr.count_table(o, want, 8, fps)[0][:, :G - 1])
            assert lib.mk_query_panel(ix._h, ptrs, lens, starts, 2, got.ctypes.data, None) == MK_OK
            seens = pr.seen_per_sample(o, [s.queries[:1], s.queries[1:3]])
            np.testing.assert_array_equal(got[:2], pr.covered(o, seens, fps)[:, :G - 1])
    finally:
        ix.close()


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    lib = ix._lib
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        cov, cells = ix.panel([reads, [], reads[:1]])
        assert cov.shape == (3, 0) and cells.tolist() == [0, 0, 0]
        marks = np.arange(7, 11, dtype=np.uint32)
        out, n = marks.copy(), np.full(3, 99, np.uint64)
        ptrs, lens = (C.c_char_p * 2)(*reads), (C.c_uint64 * 2)(*[len(r) for r in reads])
        starts = (C.c_uint64 * 3)(0, 1, 2)
        assert lib.mk_query_panel(ix._h, ptrs, lens, starts, 2, out.ctypes.data, n.ctypes.data) == MK_OK
        assert n.tolist() == [0, 0, 99]
        assert lib.mk_query_panel(ix._h, ptrs, lens, starts, 2, None, None) == MK_OK
        np.testing.assert_array_equal(out, marks)                          # covered is not written
        table = (np.arange(131072) % 256).astype(np.uint8)
        with DevBuf(ix, 131072) as tab, Uploaded(ix, reads) as qs:
            assert lib.mk_panel_bytes(ix._h) == 131072
            tab.upload(table)
            assert run(ix, qs, 2, tab) == MK_OK
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(tab.download(), table)
            n = np.full(4, 99, np.uint64)
            assert lib.mk_panel_count(ix._h, tab.p, 3, None, n.ctypes.data) == MK_OK      # cells are still the table's
            assert n.tolist() == [int(((table >> s) & 1).sum()) for s in range(3)] + [99]
    finally:
        ix.close()
