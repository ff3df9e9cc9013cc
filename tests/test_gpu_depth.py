"""mk_depth_bytes / mk_depth_reset / mk_qset_run_depth / mk_depth_profile / mk_query_depth and Miekki.depth: depth of coverage
-- per (partition, value) cell the number of queries whose gated sketch holds it, capped at 255, and per indexed genome the
covered fingerprints, the sum and the lower median of its cells' counters -- must be, byte for byte and count for count, what
tests/depth_ref.py makes of the ORACLE's gated sketches and stored columns (the median there from a sort, not a bisection)."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import cover_ref as cr
import depth_ref as dr
import synth
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_STATE = 0, -1, -5
WIDTHS = [8, 16]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """a tr.Sample with the oracle's counters and profile of all its queries, each computed once"""

    def __init__(self, *args, **kw):
        self.s = s = tr.Sample(*args, **kw)
        self.o = o = s.o
        self.h, self.bits, self.P, self.G = o.number_minimizer_log2, o.number_bit_minimizer, o.P, o.index_size
        self.fps = cr.stored(o)
        self.mult = dr.mult(o, s.queries)
        self.tab = dr.table(self.mult)
        self.med, self.sum, self.cov = dr.profile(o, self.tab, self.fps)
        self.cells, self.sat = int((self.tab > 0).sum()), int((self.tab == 255).sum())
        self.nbytes = self.P << self.bits

    def profile(self, tab):
        return dr.profile(self.o, tab, self.fps) + (int((tab > 0).sum()), int((tab == 255).sum()))


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
    """a depth table of the index's own size, reset"""

    def __init__(self, ix):
        n = ix._lib.mk_depth_bytes(ix._h)
        assert n == 1 << ix._p.h << ix._p.fp_bits
        DevBuf.__init__(self, ix, n)
        check(ix._lib.mk_depth_reset(ix._h, self.p))


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


DEPTH = np.dtype([("sum", np.uint64), ("covered", np.uint32), ("median", np.uint32)])


def run(ix, qs, tab):
    return ix._lib.mk_qset_run_depth(ix._h, qs, tab.p)


def profile(ix, tab, G=None):
    """mk_depth_profile: (median, sum, covered, cells, saturated)"""
    G = ix.index_size if G is None else G
    assert DEPTH.itemsize == 16
    d = np.zeros(G, DEPTH)
    d["sum"], d["covered"], d["median"] = 0xdead, 0xdead, 0xdead
    cells, sat = C.c_uint64(0xdead), C.c_uint64(0xdead)
    check(ix._lib.mk_depth_profile(ix._h, tab.p, d.ctypes.data, C.byref(cells), C.byref(sat)))
    return d["median"].copy(), d["sum"].copy(), d["covered"].copy(), int(cells.value), int(sat.value)


def pieces(ix, seqs):
    """mk_dev_alloc, mk_depth_reset, mk_qset_upload, mk_qset_run_depth, mk_depth_profile"""
    with Table(ix) as tab:
        with Uploaded(ix, seqs) as qs:
            check(run(ix, qs, tab))
        return profile(ix, tab)


def same(got, want):
    """(median, sum, covered, cells, saturated) against the yardstick's"""
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint64 and got[2].dtype == np.uint32
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], want[0])
    assert tuple(got[3:]) == tuple(want[3:])


@pytest.mark.parametrize("chunk", [None, "16"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_marks_are_the_reference_table(indexes, monkeypatch, bits, chunk):
    """the downloaded table, byte for byte: the set in one pass and in two halves, and a reset in between; no scan is launched,
    so chunks of 16 queries make no difference"""
    w, ix = indexes(bits)
    if chunk:
        monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", chunk)
    q = w.s.queries
    ix.reset_stats()
    before = ix.stats()["scan_launches"]
    with Table(ix) as tab:
        assert tab.nbytes == w.nbytes
        with Uploaded(ix, q) as qs:
            check(run(ix, qs, tab))
        np.testing.assert_array_equal(tab.download(), w.tab)
        check(ix._lib.mk_depth_reset(ix._h, tab.p))
        assert not tab.download().any()
        for part in (q[:300], q[300:]):
            with Uploaded(ix, part) as qs:
                check(run(ix, qs, tab))
        np.testing.assert_array_equal(tab.download(), w.tab)
    st = ix.stats()
    assert st["scan_launches"] == before and st["sketch_ms"] > 0 and st["filter_ms"] > 0


@pytest.mark.parametrize("filt", [None, "0"])
def test_five_passes_saturate_some_cells_and_not_their_neighbours(indexes, monkeypatch, filt):
    """the 8-bit set run five times into one table: passes accumulate, the largest counter (65) passes the cap and stays at
    255, and the bytes beside it in its dword are exactly theirs -- with the plain load in front of the compare-and-swap and
    without it"""
    w, ix = indexes(8)
    if filt:
        monkeypatch.setenv("MIEKKI_DEPTH_FILTER", filt)
    want = dr.table(w.mult * 5)
    d = want.reshape(-1, 4)
    assert (((d == 255).any(1)) & (((d > 0) & (d < 255)).any(1))).any()   # (on the yardstick)
    with Table(ix) as tab:
        with Uploaded(ix, w.s.queries) as qs:
            for _ in range(5):
                check(run(ix, qs, tab))
        np.testing.assert_array_equal(tab.download(), want)
        same(profile(ix, tab), w.profile(want))


@pytest.mark.parametrize("rows", [None, "24", "44"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_profile_like_the_oracle(indexes, monkeypatch, bits, rows):
    """Miekki.depth and the pieces, in the default chunks of rows, in chunks of 24 rows, which do not divide 512, and in chunks
    of 44: at 8 bits a whole stage of the table (32 rows), then a partial one of 12 whose last group of rows holds 4"""
    w, ix = indexes(bits)
    if rows:
        monkeypatch.setenv("MIEKKI_DEPTH_ROWS", rows)
    want = (w.med, w.sum, w.cov, w.cells, w.sat)
    got = ix.depth(w.s.queries)
    assert got[0].shape == got[1].shape == got[2].shape == (w.G,)
    same(got, want)
    same(pieces(ix, w.s.queries), want)


@pytest.fixture(scope="module")
def single_rows(samples, tmp_path_factory):
    """mk_depth_profile over the yardstick's table with MIEKKI_DEPTH_ROWS=1 in fresh processes (tests/depth_worker.py), both
    widths at once"""
    d = tmp_path_factory.mktemp("depth_rows")
    procs = {}
    for bits in WIDTHS:
        w = samples(bits)
        with open(d / f"job_{bits}.pkl", "wb") as f:
            pickle.dump({"par": w.s.c.par, "seqs": w.s.c.seqs, "table": w.tab}, f)
        env = dict(os.environ, MIEKKI_DEPTH_ROWS="1")
        procs[bits] = subprocess.Popen([sys.executable, os.path.join(HERE, "depth_worker.py"), str(d / f"job_{bits}.pkl"), str(d / f"out_{bits}.npz")],
                                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for bits, p in procs.items():
        text = p.communicate(timeout=300)[0]
        assert p.returncode == 0, text.decode(errors="replace")[-3000:]
        out[bits] = dict(np.load(d / f"out_{bits}.npz"))
    return out


@pytest.mark.parametrize("bits", WIDTHS)
def test_chunks_of_one_row_in_a_fresh_process(samples, single_rows, bits):
    w, r = samples(bits), single_rows[bits]
    same((r["median"], r["sum"], r["covered"], int(r["cells"]), int(r["saturated"])), (w.med, w.sum, w.cov, w.cells, w.sat))


@pytest.mark.parametrize("bits", WIDTHS)
def test_one_query_has_depth_one(indexes, bits):
    """for a set of one query every counter is at most 1, the median is 1 where covered, and sum = covered = query_sequence's
    row: a short read, a whole genome, and two genomes in a row (beyond the in-LDS sketch: a dense query)"""
    w, ix = indexes(bits)
    s = w.s
    for q in (s.reads[0], s.c.seqs[64], s.c.seqs[7] + s.c.seqs[8]):
        row = w.o.query_sequence(q)[0]
        with Table(ix) as tab:
            with Uploaded(ix, [q]) as qs:
                check(run(ix, qs, tab))
            assert tab.download().max() == 1
        med, total, cov, cells, sat = ix.depth([q])
        np.testing.assert_array_equal(cov, row)
        np.testing.assert_array_equal(total, row.astype(np.uint64))
        np.testing.assert_array_equal(med, (row > 0).astype(np.uint32))
        assert cells == int((w.o.minhash_sketch_partition_solid_kmers(q) != cr.empty_of(w.o)).sum()) and sat == 0


@pytest.mark.parametrize("bits", WIDTHS)
def test_mixed_set_with_dense_queries(indexes, bits):
    """short reads next to queries beyond the short path (dense at -h 9): a shell over two parts, marked part by part"""
    w, ix = indexes(bits)
    s = w.s
    q = s.reads[:70] + [s.c.seqs[7] + s.c.seqs[8], s.c.seqs[100] + s.c.seqs[101][:2500]] + s.reads[70:90] + [s.c.seqs[3] * 2]
    assert sum(len(x) > s.c.K + 4096 for x in q) == 3
    want = dr.table(dr.mult(w.o, q))
    assert want.max() >= 2
    with Table(ix) as tab:
        with Uploaded(ix, q) as qs:
            check(run(ix, qs, tab))
        np.testing.assert_array_equal(tab.download(), want)
        same(profile(ix, tab), w.profile(want))


@pytest.mark.parametrize("bits", WIDTHS)
def test_every_indexed_genome_as_a_query(indexes, bits):
    """mk_qset_from_index: covered is the sketch size, and a cell's counter the number of genomes that hold it, capped"""
    w, ix = indexes(bits)
    live = w.fps != cr.empty_of(w.o)
    holders = np.zeros((w.P, 1 << bits), np.int64)
    np.add.at(holders, (np.nonzero(live)[0], w.fps[live]), 1)
    want = dr.table(holders)
    assert want.max() >= 2
    with Table(ix) as tab, FromIndex(ix, np.arange(w.G)) as qs:
        check(run(ix, qs, tab))
        np.testing.assert_array_equal(tab.download(), want)
        got = profile(ix, tab)
    np.testing.assert_array_equal(got[2], w.o.sketch_size)
    same(got, w.profile(want))


@pytest.mark.parametrize("bits", WIDTHS)
def test_profile_alone_on_uploaded_tables(indexes, bits):
    w, ix = indexes(bits)
    ss = w.o.sketch_size
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(np.full(w.nbytes, 255, np.uint8))                        # every stored fingerprint but `empty`, at the cap
        med, total, cov, cells, sat = profile(ix, tab)
        np.testing.assert_array_equal(cov, ss)
        np.testing.assert_array_equal(total, 255 * ss.astype(np.uint64))
        np.testing.assert_array_equal(med, np.where(ss > 0, 255, 0))
        assert cells == sat == w.P << bits
        tab.upload(np.ones(w.nbytes, np.uint8))
        med, total, cov, cells, sat = profile(ix, tab)
        np.testing.assert_array_equal(cov, ss)
        np.testing.assert_array_equal(total, ss.astype(np.uint64))
        np.testing.assert_array_equal(med, np.where(ss > 0, 1, 0))
        assert (cells, sat) == (w.P << bits, 0)
        only_empty = np.zeros((w.P, 1 << bits), np.uint8)
        only_empty[:, cr.empty_of(w.o)] = 200
        tab.upload(only_empty.reshape(-1))                                  # a genome without a fingerprint never counts
        med, total, cov, cells, sat = profile(ix, tab)
        assert not med.any() and not total.any() and not cov.any() and (cells, sat) == (w.P, 0)
        zero_only = np.zeros((w.P, 1 << bits), np.uint8)
        zero_only[:, 0] = 7                                                 # value 0 everywhere: the rows' zero padding is not genomes
        tab.upload(zero_only.reshape(-1))
        med, total, cov, cells, sat = profile(ix, tab)
        at0 = (w.fps == 0).sum(0)
        np.testing.assert_array_equal(cov, at0.astype(np.uint32))
        np.testing.assert_array_equal(total, 7 * at0.astype(np.uint64))
        np.testing.assert_array_equal(med, np.where(at0 > 0, 7, 0))
        assert (cells, sat) == (w.P, 0)
        noise = np.random.default_rng(3).integers(0, 256, w.nbytes, dtype=np.uint8)
        want = w.profile(noise)
        assert len(set(want[0].tolist())) >= 20                             # the bisection decides both ways at every step
        tab.upload(noise)
        same(profile(ix, tab), want)


class Large:
    """-h 17, 40 genomes of 200 kb: sketches beyond 65,535 partitions, and sums beyond 16 bits per chunk.  The oracle's sketch
    sizes and the index, once per width."""

    K, H, N, LEN = 31, 17, 40, 200_000

    def __init__(self, hip, bits):
        from oracle import oracle as orc
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


@pytest.mark.parametrize("rows", [None, "131072"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_counts_reach_the_sketch_size_beyond_16_bits(large, monkeypatch, bits, rows):
    """an all-255 table: covered is the sketch size, above 65,535, and sum 255 times that -- in the default chunks and with
    every row in one chunk"""
    l = large(bits)
    ix, ss = l.ix, l.o.sketch_size
    assert ss.min() > 65_535
    if rows:
        monkeypatch.setenv("MIEKKI_DEPTH_ROWS", rows)
    nbytes = 1 << l.H << bits
    full = np.full(min(nbytes, 16 << 20), 255, np.uint8)
    with DevBuf(ix, nbytes) as tab:
        for at in range(0, nbytes, full.nbytes):
            tab.upload(full, at)
        med, total, cov, cells, sat = profile(ix, tab)
    np.testing.assert_array_equal(cov, ss)
    np.testing.assert_array_equal(total, 255 * ss.astype(np.uint64))
    assert (med == 255).all() and cells == sat == 1 << l.H << bits


@pytest.mark.parametrize("bits", WIDTHS)
def test_a_long_sparse_read_has_depth_one(large, bits):
    """10 kb against 2^17 partitions: beyond the in-LDS sketch and not dense -- the long path's entry list"""
    l = large(bits)
    q = l.seqs[5][30_000:40_000]
    row = l.o.query_sequence(q)[0]
    med, total, cov, cells, sat = l.ix.depth([q])
    np.testing.assert_array_equal(cov, row)
    np.testing.assert_array_equal(total, row.astype(np.uint64))
    np.testing.assert_array_equal(med, (row > 0).astype(np.uint32))
    assert cov[5] > 5000 and sat == 0 and cells == int((l.o.minhash_sketch_partition_solid_kmers(q) != cr.empty_of(l.o)).sum())


def test_second_slice_of_mk_query_depth(indexes):
    """2^18 + 5 reads, 64 distinct ones repeated 4,096 times and more: mk_query_depth marks them as two uploaded sets into one
    table, and every seen cell saturates -- under the heaviest contention the marks meet"""
    w, ix = indexes(16)
    reads, queries, times = synth.two_slices(w.s.c.seqs, 22)
    assert len(queries) == (1 << 18) + 5 and min(times) >= 255
    seen = cr.seen(w.o, reads)
    cov = cr.covered(w.o, seen, w.fps)
    assert (cov > 0).sum() >= 2                                             # (on the oracle: nothing passes on zeros)
    med, total, got, cells, sat = ix.depth(queries)
    np.testing.assert_array_equal(got, cov)
    np.testing.assert_array_equal(total, 255 * cov.astype(np.uint64))
    np.testing.assert_array_equal(med, np.where(cov > 0, 255, 0))
    assert cells == sat == int(seen.sum())


@pytest.mark.parametrize("bits", WIDTHS)
def test_cold_rows_raw_and_packed(hip, samples, monkeypatch, bits):
    """1 MiB of a 2 MiB matrix in HBM (a reservation doubles the rows' pitch), the other rows in host memory: read where they
    lie; then packed (compress_index), which the profile unpacks first"""
    w = samples(bits)
    want = (w.med, w.sum, w.cov, w.cells, w.sat)
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = hip.Miekki(*w.s.c.par)
    try:
        ix.reserve(4096 * 8 // bits)
        for i in range(0, w.G, 64):
            ix.insert_sequences(w.s.c.seqs[i:i + 64])
        same(ix.depth(w.s.queries), want)
        raw, packed = ix.compress_index()
        assert raw >= 1 << 20                                              # (there are cold rows)
        same(pieces(ix, w.s.queries), want)
        ix.compress_index()
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.tab)
            same(profile(ix, tab), want)
    finally:
        ix.close()


def test_results_are_by_local_genome(hip, samples):
    """genome_id_base 1000: depth[j] is local genome j's, whatever ids the context reports"""
    w = samples(8)
    want = (w.med, w.sum, w.cov, w.cells, w.sat)
    ix = w.s.a.build(hip, genome_id_base=1000)
    try:
        same(ix.depth(w.s.queries), want)
        same(pieces(ix, w.s.queries), want)
    finally:
        ix.close()


def test_refusals_leave_the_table_alone(hip, samples):
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
        d = np.zeros(G, DEPTH)
        cells, sat = C.c_uint64(0), C.c_uint64(0)
        with DevBuf(ix, w.nbytes) as tab, Uploaded(ix, s.queries[:40]) as qs, Uploaded(ix, []) as none, FromIndex(ix, np.arange(G)) as own:
            tab.upload(marks)
            assert lib.mk_qset_run_depth(None, qs, tab.p) == MK_ERR_ARG
            assert lib.mk_qset_run_depth(ix._h, None, tab.p) == MK_ERR_ARG
            assert lib.mk_qset_run_depth(ix._h, qs, None) == MK_ERR_ARG
            assert lib.mk_depth_reset(ix._h, None) == MK_ERR_ARG
            assert lib.mk_depth_reset(None, tab.p) == MK_ERR_ARG
            assert lib.mk_depth_profile(ix._h, None, d.ctypes.data, C.byref(cells), C.byref(sat)) == MK_ERR_ARG
            assert lib.mk_depth_profile(ix._h, tab.p, None, C.byref(cells), C.byref(sat)) == MK_ERR_ARG
            assert lib.mk_query_depth(ix._h, None, None, 3, d.ctypes.data, C.byref(cells), C.byref(sat)) == MK_ERR_ARG
            ptrs, lens = (C.c_char_p * 2)(*s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in s.queries[:2]])
            assert lib.mk_query_depth(ix._h, ptrs, lens, 2, None, C.byref(cells), C.byref(sat)) == MK_ERR_ARG
            assert run(ix, none, tab) == MK_OK                              # an empty set
            ix.select(np.arange(G - 1))                                     # `own` names what was there before
            assert run(ix, own, tab) == MK_ERR_STATE
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(tab.download(), marks)
            assert not d["covered"].any() and not d["sum"].any() and cells.value == 0 and sat.value == 0
            check(run(ix, qs, tab))                                         # ... and an uploaded set still runs: its counts are added
            want = dr.table(marks.astype(np.int64).reshape(w.P, -1) + dr.mult(o, s.queries[:40]))
            np.testing.assert_array_equal(tab.download(), want)
            check(lib.mk_depth_profile(ix._h, tab.p, d.ctypes.data, None, None))   # cells and saturated may be NULL
            med, total, cov = dr.profile(o, want, fps)
            np.testing.assert_array_equal(d["covered"][:G - 1], cov[:G - 1])
            np.testing.assert_array_equal(d["sum"][:G - 1], total[:G - 1])
            np.testing.assert_array_equal(d["median"][:G - 1], med[:G - 1])
    finally:
        ix.close()


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        med, total, cov, cells, sat = ix.depth(reads)
        assert med.shape == total.shape == cov.shape == (0,) and (cells, sat) == (0, 0)
        marks = np.arange(7, 11, dtype=np.uint64)
        out, n, f = marks.copy(), C.c_uint64(99), C.c_uint64(99)
        ptrs, lens = (C.c_char_p * 2)(*reads), (C.c_uint64 * 2)(*[len(r) for r in reads])
        assert ix._lib.mk_query_depth(ix._h, ptrs, lens, 2, out.ctypes.data, C.byref(n), C.byref(f)) == MK_OK
        assert n.value == 0 and f.value == 0
        assert ix._lib.mk_query_depth(ix._h, ptrs, lens, 2, None, None, None) == MK_OK
        np.testing.assert_array_equal(out, marks)                          # depth is not written
        table = (np.arange(131072) % 256).astype(np.uint8)
        with DevBuf(ix, 131072) as tab, Uploaded(ix, reads) as qs:
            assert ix._lib.mk_depth_bytes(ix._h) == 131072
            tab.upload(table)
            assert run(ix, qs, tab) == MK_OK
            check(ix._lib.mk_sync(ix._h))
            np.testing.assert_array_equal(tab.download(), table)
            n, f = C.c_uint64(0), C.c_uint64(0)
            assert ix._lib.mk_depth_profile(ix._h, tab.p, None, C.byref(n), C.byref(f)) == MK_OK
            assert (n.value, f.value) == (int((table > 0).sum()), int((table == 255).sum()))
    finally:
        ix.close()


def test_agreement_with_the_cover_that_exists(hip):
    """no oracle: strain reads at -h 14.  covered from mk_depth_profile is mk_cover_count's over the same reads, the table's
    non-zero bytes are the cover table's bits, and sum is at least covered and at most the reads times covered"""
    SP, ST, SL, PPM = 3, 48, 50_000, 3000
    G, H = SP * ST, 14
    P = 1 << H
    seqs = [synth.strain_device(g, ST, PPM, 0, SL) for g in range(G)]
    ix = hip.Miekki(31, H, 8, 33, 200)
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
        seen = DevBuf(ix, lib.mk_cover_bytes(ix._h))
        with Table(ix) as tab, seen:
            check(lib.mk_cover_reset(ix._h, seen.p))
            with Uploaded(ix, reads) as qs:
                check(run(ix, qs, tab))
                check(lib.mk_qset_run_cover(ix._h, qs, seen.p))
            mult = tab.download().reshape(P, 256)
            bits = cr.unpack(seen.download().view(np.uint32), P, 8)
            med, total, cov, cells, sat = profile(ix, tab)
            cov2, cells2 = np.zeros(G, np.uint32), C.c_uint64(0)
            check(lib.mk_cover_count(ix._h, seen.p, cov2.ctypes.data, C.byref(cells2)))
        np.testing.assert_array_equal(mult > 0, bits)
        np.testing.assert_array_equal(cov, cov2)
        assert cells == cells2.value == bits.sum() and sat == 0 and cov.max() > 900 and mult.max() >= 2
        assert (total >= cov).all() and (total <= 300 * cov.astype(np.uint64)).all() and (total > cov).any()
        assert ((med >= 1) == (cov > 0)).all() and (med <= mult.max()).all()
    finally:
        ix.close()
