"""mk_cover_bytes / mk_cover_reset / mk_qset_run_cover / mk_cover_count / mk_query_cover and Miekki.cover: breadth of coverage
-- per indexed genome, how many of its stored fingerprints turn up in the gated sketch of some query -- must be, bit for bit
and count for count, what tests/cover_ref.py makes of the ORACLE's gated sketches and stored columns."""
import ctypes as C

import numpy as np
import pytest

import cover_ref as cr
import synth
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_STATE = 0, -1, -5
WIDTHS = [8, 16]


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """a tr.Sample with the oracle's table and counts of all its queries, each computed once"""

    def __init__(self, *args, **kw):
        self.s = s = tr.Sample(*args, **kw)
        self.o = o = s.o
        self.h, self.bits, self.P, self.G = o.number_minimizer_log2, o.number_bit_minimizer, o.P, o.index_size
        self.fps = cr.stored(o)
        self.seen = cr.seen(o, s.queries)
        self.words = cr.pack(self.seen)
        self.cov = cr.covered(o, self.seen, self.fps)
        self.cells = int(self.seen.sum())
        self.nbytes = (self.P << self.bits) >> 3


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

    def download(self, arr=None):
        arr = np.zeros(self.nbytes // 4, np.uint32) if arr is None else arr
        check(self.ix._lib.mk_dev_download(self.ix._h, arr.ctypes.data, self.p, arr.nbytes))
        return arr


class Table(DevBuf):
    """a cover table of the index's own size, reset"""

    def __init__(self, ix):
        n = ix._lib.mk_cover_bytes(ix._h)
        assert n == (1 << ix._p.h << ix._p.fp_bits) >> 3
        DevBuf.__init__(self, ix, n)
        check(ix._lib.mk_cover_reset(ix._h, self.p))


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


def run(ix, qs, tab):
    return ix._lib.mk_qset_run_cover(ix._h, qs, tab.p)


def count(ix, tab, G=None):
    G = ix.index_size if G is None else G
    cov, cells = np.full(G, 0xdead, np.uint32), C.c_uint64(0xdead)
    check(ix._lib.mk_cover_count(ix._h, tab.p, cov.ctypes.data, C.byref(cells)))
    return cov, int(cells.value)


def pieces(ix, seqs):
    """mk_dev_alloc, mk_cover_reset, mk_qset_upload, mk_qset_run_cover, mk_cover_count"""
    with Table(ix) as tab:
        with Uploaded(ix, seqs) as qs:
            check(run(ix, qs, tab))
        return count(ix, tab)


@pytest.mark.parametrize("bits", WIDTHS)
def test_sample_preconditions_from_the_oracle_alone(samples, bits):
    """what the definition promises, on the oracle alone: for the 620 reads every genome's covered lies between the maximum
    and the sum of its score column, for most of them strictly; for one query covered IS its score row"""
    w = samples(bits)
    s, o = w.s, w.o
    ss = o.sketch_size.astype(np.int64)
    seen = cr.seen(o, s.reads)
    cov = cr.covered(o, seen, w.fps).astype(np.int64)
    rows = s.read_rows.astype(np.int64)
    mx, sm = rows.max(0), rows.sum(0)
    print("cells", int(seen.sum()), "strictly between", int(((mx < cov) & (cov < sm)).sum()), "zero", int((cov == 0).sum()))
    assert (mx <= cov).all() and (cov <= np.minimum(sm, ss)).all()
    assert ((mx < cov) & (cov < sm)).sum() >= (1000 if bits == 8 else 500)
    live = [int((o.minhash_sketch_partition_solid_kmers(q) != cr.empty_of(o)).sum()) for q in s.reads]
    assert max(live) <= seen.sum() <= min(sum(live), o.P << bits) and seen.sum() > 20_000
    assert not seen[:, cr.empty_of(o)].any()
    lens = [len(q) for q in s.queries]
    for q in (int(np.argmin(lens)), int(np.argmax(lens[:len(s.reads)])), len(s.queries) - 1):       # a short read, a long one, a whole genome (8-bit)
        np.testing.assert_array_equal(cr.covered(o, cr.seen(o, [s.queries[q]]), w.fps), s.rows[q])


@pytest.mark.parametrize("chunk", [None, "16"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_marks_are_the_reference_table(indexes, monkeypatch, bits, chunk):
    """the downloaded table, bit for bit: the set in one pass, in two halves, and run twice; no scan is launched, so chunks of
    16 queries make no difference"""
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
            np.testing.assert_array_equal(tab.download(), w.words)
            check(run(ix, qs, tab))                                        # the same set again: an OR changes nothing
            np.testing.assert_array_equal(tab.download(), w.words)
        check(ix._lib.mk_cover_reset(ix._h, tab.p))
        assert not tab.download().any()
        for part in (q[:300], q[300:]):
            with Uploaded(ix, part) as qs:
                check(run(ix, qs, tab))
        np.testing.assert_array_equal(tab.download(), w.words)
    st = ix.stats()
    assert st["scan_launches"] == before and st["sketch_ms"] > 0 and st["filter_ms"] > 0


def test_second_slice_of_mk_query_cover(indexes):
    """2^18 + 5 reads, 64 distinct ones repeated: mk_query_cover marks them as two uploaded sets into one table -- an OR
    ignores repeats, so the counts are the oracle's for the 64 distinct reads"""
    w, ix = indexes(16)
    reads, queries, _ = synth.two_slices(w.s.c.seqs, 22)
    assert len(queries) == (1 << 18) + 5
    alone = [cr.covered(w.o, cr.seen(w.o, [r]), w.fps) for r in reads]
    seen = cr.seen(w.o, reads)
    want = cr.covered(w.o, seen, w.fps)
    assert all(a.any() for a in alone) and (want > 0).sum() >= 2          # (on the oracle: nothing passes on zeros)
    got, cells = ix.cover(queries)
    np.testing.assert_array_equal(got, want)
    assert cells == int(seen.sum())


@pytest.mark.parametrize("rows", [None, "24", "300"])
@pytest.mark.parametrize("bits", WIDTHS)
def test_counts_like_the_oracle(indexes, monkeypatch, bits, rows):
    """Miekki.cover and the pieces, in the default chunks of rows, in chunks of 24 rows, which do not divide 512, and in chunks
    of 300: at 8 bits a whole stage of the table (256 rows), then a partial one of 44 whose last group of rows holds 4"""
    w, ix = indexes(bits)
    if rows:
        monkeypatch.setenv("MIEKKI_COVER_ROWS", rows)
    got, cells = ix.cover(w.s.queries)
    assert got.dtype == np.uint32 and got.shape == (w.G,)
    np.testing.assert_array_equal(got, w.cov)
    assert cells == w.cells
    got, cells = pieces(ix, w.s.queries)
    np.testing.assert_array_equal(got, w.cov)
    assert cells == w.cells


@pytest.mark.parametrize("bits", WIDTHS)
def test_one_query_is_its_score_row(indexes, bits):
    """for a set of one query covered is query_sequence's row: a short read, a whole genome, and two genomes in a row (beyond
    the in-LDS sketch: a dense query)"""
    w, ix = indexes(bits)
    s = w.s
    for q in (s.reads[0], s.c.seqs[64], s.c.seqs[7] + s.c.seqs[8]):
        row = ix.query_sequences([q])[0]
        got, cells = ix.cover([q])
        np.testing.assert_array_equal(got, row)
        np.testing.assert_array_equal(got, w.o.query_sequence(q)[0])
        assert cells == int((w.o.minhash_sketch_partition_solid_kmers(q) != cr.empty_of(w.o)).sum())


@pytest.mark.parametrize("bits", WIDTHS)
def test_mixed_set_with_dense_queries(indexes, bits):
    """short reads next to queries beyond the short path (dense at -h 9): a shell over two parts, marked part by part"""
    w, ix = indexes(bits)
    s = w.s
    q = s.reads[:70] + [s.c.seqs[7] + s.c.seqs[8], s.c.seqs[100] + s.c.seqs[101][:2500]] + s.reads[70:90] + [s.c.seqs[3] * 2]
    assert sum(len(x) > s.c.K + 4096 for x in q) == 3
    seen = cr.seen(w.o, q)
    with Table(ix) as tab:
        with Uploaded(ix, q) as qs:
            check(run(ix, qs, tab))
        np.testing.assert_array_equal(tab.download(), cr.pack(seen))
        got, cells = count(ix, tab)
    np.testing.assert_array_equal(got, cr.covered(w.o, seen, w.fps))
    assert cells == seen.sum()


@pytest.mark.parametrize("bits", WIDTHS)
def test_every_indexed_genome_covers_every_sketch(indexes, bits):
    w, ix = indexes(bits)
    with Table(ix) as tab, FromIndex(ix, np.arange(w.G)) as qs:
        check(run(ix, qs, tab))
        got, cells = count(ix, tab)
    np.testing.assert_array_equal(got, w.o.sketch_size)
    live = w.fps != cr.empty_of(w.o)
    want = np.zeros((w.P, 1 << bits), bool)
    want[np.nonzero(live)[0], w.fps[live]] = True
    assert cells == want.sum()


@pytest.mark.parametrize("bits", WIDTHS)
def test_count_alone_on_uploaded_tables(indexes, bits):
    w, ix = indexes(bits)
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(np.full(w.nbytes // 4, 0xffffffff, np.uint32))          # all ones: every stored fingerprint but `empty`
        got, cells = count(ix, tab)
        np.testing.assert_array_equal(got, w.o.sketch_size)
        assert cells == w.P << bits
        only_empty = np.zeros((w.P, 1 << bits), bool)
        only_empty[:, cr.empty_of(w.o)] = True
        tab.upload(cr.pack(only_empty))                                     # a genome without a fingerprint never counts
        got, cells = count(ix, tab)
        assert not got.any() and cells == w.P
        tab.upload(np.zeros(w.nbytes // 4, np.uint32))
        got, cells = count(ix, tab)
        assert not got.any() and cells == 0
        zero_only = np.zeros((w.P, 1 << bits), bool)
        zero_only[:, 0] = True                                              # value 0 everywhere: the rows' zero padding is not genomes
        tab.upload(cr.pack(zero_only))
        got, cells = count(ix, tab)
        np.testing.assert_array_equal(got, (w.fps == 0).sum(0).astype(np.uint32))
        assert cells == w.P


class Large:
    """-h 17, 40 genomes of 200 kb: sketches beyond 65,535 partitions -- the smallest shape at which packed 8-bit or 16-bit
    accumulators of the count pass could overflow.  The oracle's sketch sizes and the index, once per width."""

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
    """an all-ones table: covered is the sketch size, above 65,535 -- in the default chunks and with every row in one chunk"""
    l = large(bits)
    ix, ss = l.ix, l.o.sketch_size
    assert ss.min() > 65_535
    if rows:
        monkeypatch.setenv("MIEKKI_COVER_ROWS", rows)
    nbytes = (1 << l.H << bits) >> 3
    ones = np.full(min(nbytes, 16 << 20) // 4, 0xffffffff, np.uint32)
    with DevBuf(ix, nbytes) as tab:
        for at in range(0, nbytes, ones.nbytes):
            tab.upload(ones, at)
        got, cells = count(ix, tab)
    np.testing.assert_array_equal(got, ss)
    assert cells == 1 << l.H << bits


@pytest.mark.parametrize("bits", WIDTHS)
def test_a_long_sparse_read_is_its_score_row(large, bits):
    """10 kb against 2^17 partitions: beyond the in-LDS sketch and not dense -- the long path's entry list"""
    l = large(bits)
    q = l.seqs[5][30_000:40_000]
    got, cells = l.ix.cover([q])
    np.testing.assert_array_equal(got, l.o.query_sequence(q)[0])
    np.testing.assert_array_equal(got, l.ix.query_sequences([q])[0])
    assert got[5] > 5000 and cells == int((l.o.minhash_sketch_partition_solid_kmers(q) != cr.empty_of(l.o)).sum())


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
        got, cells = ix.cover(w.s.queries)
        np.testing.assert_array_equal(got, w.cov)
        assert cells == w.cells
        raw, packed = ix.compress_index()
        assert raw >= 1 << 20                                              # (there are cold rows)
        np.testing.assert_array_equal(pieces(ix, w.s.queries)[0], w.cov)
        ix.compress_index()
        with DevBuf(ix, w.nbytes) as tab:
            tab.upload(w.words)
            np.testing.assert_array_equal(count(ix, tab)[0], w.cov)
    finally:
        ix.close()


def test_counts_are_by_local_genome(hip, samples):
    """genome_id_base 1000: covered[j] is local genome j's, whatever ids the context reports"""
    w = samples(8)
    ix = w.s.a.build(hip, genome_id_base=1000)
    try:
        got, cells = ix.cover(w.s.queries)
        np.testing.assert_array_equal(got, w.cov)
        got2, cells2 = pieces(ix, w.s.queries)
        np.testing.assert_array_equal(got2, w.cov)
        assert cells == cells2 == w.cells
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
        rng = np.random.default_rng(3)
        marks = rng.integers(0, 1 << 32, w.nbytes // 4, dtype=np.uint64).astype(np.uint32)
        cov = np.zeros(G, np.uint32)
        cells = C.c_uint64(0)
        with DevBuf(ix, w.nbytes) as tab, Uploaded(ix, s.queries[:40]) as qs, Uploaded(ix, []) as none, FromIndex(ix, np.arange(G)) as own:
            tab.upload(marks)
            assert lib.mk_qset_run_cover(None, qs, tab.p) == MK_ERR_ARG
            assert lib.mk_qset_run_cover(ix._h, None, tab.p) == MK_ERR_ARG
            assert lib.mk_qset_run_cover(ix._h, qs, None) == MK_ERR_ARG
            assert lib.mk_cover_reset(ix._h, None) == MK_ERR_ARG
            assert lib.mk_cover_reset(None, tab.p) == MK_ERR_ARG
            assert lib.mk_cover_count(ix._h, None, cov.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            assert lib.mk_cover_count(ix._h, tab.p, None, C.byref(cells)) == MK_ERR_ARG
            assert lib.mk_query_cover(ix._h, None, None, 3, cov.ctypes.data, C.byref(cells)) == MK_ERR_ARG
            ptrs, lens = (C.c_char_p * 2)(*s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in s.queries[:2]])
            assert lib.mk_query_cover(ix._h, ptrs, lens, 2, None, C.byref(cells)) == MK_ERR_ARG
            assert run(ix, none, tab) == MK_OK                              # an empty set
            ix.select(np.arange(G - 1))                                     # `own` names what was there before
            assert run(ix, own, tab) == MK_ERR_STATE
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(tab.download(), marks)
            assert not cov.any() and cells.value == 0
            check(run(ix, qs, tab))                                         # ... and an uploaded set still runs: its bits are OR-ed in
            want = marks | cr.pack(cr.seen(o, s.queries[:40]))
            np.testing.assert_array_equal(tab.download(), want)
            check(lib.mk_cover_count(ix._h, tab.p, cov.ctypes.data, None))  # cells may be NULL
            np.testing.assert_array_equal(cov[:G - 1], cr.covered(o, cr.unpack(want, w.P, 8), fps)[:G - 1])
    finally:
        ix.close()


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        got, cells = ix.cover(reads)
        assert got.shape == (0,) and cells == 0
        marks = np.arange(7, 11, dtype=np.uint32)
        out, n = marks.copy(), C.c_uint64(99)
        ptrs, lens = (C.c_char_p * 2)(*reads), (C.c_uint64 * 2)(*[len(r) for r in reads])
        assert ix._lib.mk_query_cover(ix._h, ptrs, lens, 2, out.ctypes.data, C.byref(n)) == MK_OK
        assert n.value == 0
        assert ix._lib.mk_query_cover(ix._h, ptrs, lens, 2, None, None) == MK_OK
        np.testing.assert_array_equal(out, marks)                          # covered is not written
        table = np.arange(4096, dtype=np.uint32)
        with DevBuf(ix, 16384) as tab, Uploaded(ix, reads) as qs:
            assert ix._lib.mk_cover_bytes(ix._h) == 16384
            tab.upload(table)
            assert run(ix, qs, tab) == MK_OK
            check(ix._lib.mk_sync(ix._h))
            np.testing.assert_array_equal(tab.download(), table)
            n = C.c_uint64(0)
            assert ix._lib.mk_cover_count(ix._h, tab.p, None, C.byref(n)) == MK_OK
            assert n.value == int(np.unpackbits(table.view(np.uint8)).sum())
    finally:
        ix.close()


def test_agreement_with_the_scans_that_exist(hip):
    """no oracle: strain reads at -h 14.  The table's distinct values per partition, laid out as columns of virtual genomes
    (slot j of partition p = the j-th seen value, or empty), are queries mk_qset_from_columns takes; values within a
    partition are distinct, so the sum of their scores over the virtual queries is covered."""
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
        with Table(ix) as tab:
            with Uploaded(ix, reads) as qs:
                check(run(ix, qs, tab))
            seen = cr.unpack(tab.download(), P, 8)
            got, cells = count(ix, tab)
        assert cells == seen.sum() and not seen[:, 255].any()
        per = seen.sum(1)
        n = int(per.max())
        assert n >= 2 and got.max() > 900
        cols = np.full((P, n), 255, np.uint8)
        p, v = np.nonzero(seen)                                            # ascending p, then v
        slot = np.arange(len(p)) - np.repeat(np.cumsum(per) - per, per)
        cols[p, slot] = v
        d_cols, d_scores, vq = C.c_void_p(), C.c_void_p(), C.c_void_p()
        scores = np.zeros((n, G), np.uint32)
        check(lib.mk_dev_alloc(ix._h, cols.nbytes, C.byref(d_cols)))
        check(lib.mk_dev_alloc(ix._h, scores.nbytes, C.byref(d_scores)))
        try:
            check(lib.mk_dev_upload(ix._h, d_cols, cols.ctypes.data, cols.nbytes))
            check(lib.mk_qset_from_columns(ix._h, d_cols, n, C.byref(vq)))
            check(lib.mk_qset_scores(ix._h, vq, 0, n, d_scores))
            check(lib.mk_sync(ix._h))
            check(lib.mk_dev_download(ix._h, scores.ctypes.data, d_scores, scores.nbytes))
            np.testing.assert_array_equal(got, scores.sum(0).astype(np.uint32))
            # ... and the virtual queries mark the table they were read from
            with Table(ix) as again:
                check(lib.mk_qset_run_cover(ix._h, vq, again.p))
                np.testing.assert_array_equal(cr.unpack(again.download(), P, 8), seen)
        finally:
            if vq:
                lib.mk_qset_free(ix._h, vq)
            lib.mk_dev_free(ix._h, d_scores)
            lib.mk_dev_free(ix._h, d_cols)
    finally:
        ix.close()
