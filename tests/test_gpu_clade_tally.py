"""mk_clade_map_* / mk_clade_tally_reset / mk_qset_run_clade_tally / mk_clade_tally_read / mk_query_clade_tally and
Miekki.clade_tally: the profile of a read set per clade of genomes, summed on the device, must be counter for counter what a
host sum makes of the ORACLE's filter_results (tests/clade_ref.py) -- for maps cut at the walks' lane and step boundaries, with
left-out genomes and gaps in the numbering, over u32 scores and over one- and two-byte partial counts."""
import ctypes as C

import numpy as np
import pytest

import clade_ref as cr
import synth
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED, MK_ERR_STATE = 0, -1, -2, -5
THRESHOLDS = [(10, 10.0), (10, 60.0), (10, 100.0)]
LAYOUTS = ["single", "one", "fine", "coarse", "masked"]
FEW = 500                          # a set below 512 short reads leaves partial counts, 512 or more u32 scores (test_gpu_tally.slab_reads_check)


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """a tr.Sample, the oracle's lists of its queries and the clade tallies of them, each computed once"""

    def __init__(self, *args, **kw):
        self.s = tr.Sample(*args, **kw)
        self.lay = cr.layouts(self.s.c.G)
        self.lists, self.memo = {}, {}

    def per_query(self, ms, mi, which="all"):
        if (ms, mi, which) not in self.lists:
            rows = {"all": self.s.rows, "few": self.s.read_rows[:FEW], "genomes": self.s.a.rows}[which]
            self.lists[ms, mi, which] = cr.per_query(self.s.o, rows, ms, mi)
        return self.lists[ms, mi, which]

    def want(self, layout, ms, mi, which="all"):
        if (layout, ms, mi, which) not in self.memo:
            self.memo[layout, ms, mi, which] = cr.clade_tally(self.per_query(ms, mi, which), self.lay[layout])
        return self.memo[layout, ms, mi, which]

    def plain(self, ms, mi, which="all"):
        return cr.plain_tally(self.per_query(ms, mi, which), self.s.c.G)


@pytest.fixture(scope="module")
def sample():
    return Wanted()


@pytest.fixture(scope="module")
def sample_index(hip, sample):
    ix = sample.s.a.build(hip)
    yield sample, ix
    ix.close()


@pytest.fixture(scope="module")
def wide_index(hip):
    """the same collection with 16-bit fingerprints: two-byte partial counts"""
    w = Wanted(fp_bits=16)
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


def make_map(ix, clade, n=None):
    """(status, handle) of mk_clade_map_create over a list of numbers / None"""
    arr = cr.as_u32(clade)
    m = C.c_void_p()
    st = ix._lib.mk_clade_map_create(ix._h, arr.ctypes.data, len(arr) if n is None else n, C.byref(m))
    return st, m


class Map:
    def __init__(self, ix, clade):
        self.ix = ix
        st, self.m = make_map(ix, clade)
        check(st)
        assert ix._lib.mk_clade_map_size(self.m) == cr.n_clades(clade)

    def __enter__(self):
        return self.m

    def __exit__(self, *a):
        self.ix._lib.mk_clade_map_free(self.ix._h, self.m)


def run(ix, qs, ms, mi, m, buf, n_clades, tally=None, n_ids=0):
    return ix._lib.mk_qset_run_clade_tally(ix._h, qs, ms, float(mi), m, buf.p, n_clades, tally.p if tally else None, n_ids)


def read(ix, buf, n_clades):
    out = np.full((n_clades, 5), 0xdead, np.uint64)
    check(ix._lib.mk_clade_tally_read(ix._h, buf.p, n_clades, out.ctypes.data))
    return out


def pieces(ix, sets, ms, mi, clade, passes=1):
    """mk_clade_map_create, mk_dev_alloc, mk_clade_tally_reset, then per set mk_qset_upload and mk_qset_run_clade_tally
    `passes` times, mk_clade_tally_read"""
    n = cr.n_clades(clade)
    with Map(ix, clade) as m, DevBuf(ix, 40 * n) as buf:
        check(ix._lib.mk_clade_tally_reset(ix._h, buf.p, n))
        for seqs in sets:
            with Uploaded(ix, seqs) as qs:
                for _ in range(passes):
                    check(run(ix, qs, ms, mi, m, buf, n))
        return read(ix, buf, n)


@pytest.mark.parametrize("ms,mi", THRESHOLDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_like_the_oracle(sample_index, layout, ms, mi):
    """the whole mixed set of 628 -- 620 short reads on u32 scores, eight whole genomes on the dense kernel's -- and its first
    500 reads on one-byte partial counts, through the pieces; the whole set in one call and from Python"""
    w, ix = sample_index
    clade = w.lay[layout]
    want = w.want(layout, ms, mi)
    assert want[:, 0].sum() > 0
    np.testing.assert_array_equal(pieces(ix, [w.s.queries], ms, mi, clade), want)
    before = ix.stats()["scan_slab_launches"]
    np.testing.assert_array_equal(pieces(ix, [w.s.reads[:FEW]], ms, mi, clade), w.want(layout, ms, mi, "few"))
    assert ix.stats()["scan_slab_launches"] > before                       # (partial counts were walked)
    ix.reset_stats()
    got = ix.clade_tally(w.s.queries, clade, ms, mi)
    assert got.dtype == np.uint64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert ix.stats()["filter_ms"] > 0                                      # the clade launches


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_byte_partial_counts(wide_index, layout):
    """16-bit fingerprints: 512 genomes per tile, the walk over two-byte partial counts; the whole mixed set in one call"""
    w, ix = wide_index
    clade = w.lay[layout]
    before = ix.stats()["scan_slab_launches"]
    for ms, mi in THRESHOLDS:
        want = w.want(layout, ms, mi, "few")
        assert want[:, 0].sum() > 0
        np.testing.assert_array_equal(pieces(ix, [w.s.reads[:FEW]], ms, mi, clade), want)
    assert ix.stats()["scan_slab_launches"] > before
    np.testing.assert_array_equal(ix.clade_tally(w.s.queries, clade, 10, 60.0), w.want(layout, 10, 60.0))


@pytest.mark.parametrize("layout", ["fine", "masked"])
def test_chunks_of_sixteen_queries(sample_index, monkeypatch, layout):
    """the chunks leave no trace: scores and partial counts in chunks of 16 queries"""
    w, ix = sample_index
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "16")
    ms, mi = 10, 60.0
    np.testing.assert_array_equal(pieces(ix, [w.s.queries], ms, mi, w.lay[layout]), w.want(layout, ms, mi))
    np.testing.assert_array_equal(pieces(ix, [w.s.reads[:FEW]], ms, mi, w.lay[layout]), w.want(layout, ms, mi, "few"))


def test_sets_from_the_index(sample_index):
    """every indexed genome as a query from its stored column, in sets of 64 ids, under `fine`: lists of whole species"""
    w, ix = sample_index
    G, clade = w.s.c.G, w.lay["fine"]
    n = cr.n_clades(clade)
    with Map(ix, clade) as m, DevBuf(ix, 40 * n) as buf:
        for ms, mi in THRESHOLDS:
            check(ix._lib.mk_clade_tally_reset(ix._h, buf.p, n))
            for g0 in range(0, G, 64):
                with FromIndex(ix, np.arange(g0, min(G, g0 + 64))) as qs:
                    check(run(ix, qs, ms, mi, m, buf, n))
            np.testing.assert_array_equal(read(ix, buf, n), w.want("fine", ms, mi, "genomes"))


def test_single_is_the_plain_tally_of_the_device(sample_index):
    """clade[j] = j: column by column mk_qset_run_tally's own output, and hits = listed"""
    w, ix = sample_index
    G = w.s.c.G
    for ms, mi in THRESHOLDS:
        got = pieces(ix, [w.s.queries], ms, mi, w.lay["single"])
        plain = ix.tally(w.s.queries, ms, mi)
        np.testing.assert_array_equal(got[:, :4], plain)
        np.testing.assert_array_equal(got[:, 4], plain[:, 0])
        one = pieces(ix, [w.s.queries], ms, mi, w.lay["one"])
        assert one.shape == (1, 5) and one[0, 0] == one[0, 1] == one[0, 2] == plain[:, 2].sum() and one[0, 4] == plain[:, 0].sum()
        assert got.shape == (G, 5)


def test_passes_accumulate_and_sets_leave_no_trace(sample_index):
    w, ix = sample_index
    ms, mi, q = 10, 60.0, w.s.queries
    for layout in ("fine", "masked"):
        want = w.want(layout, ms, mi)
        np.testing.assert_array_equal(pieces(ix, [q], ms, mi, w.lay[layout], passes=2), 2 * want)
        np.testing.assert_array_equal(pieces(ix, [q[:211], q[211:500], q[500:]], ms, mi, w.lay[layout]), want)


def scans(ix):
    st = ix.stats()
    return np.array([st["scan_launches"], st["scan_slab_launches"]], np.int64)


def test_both_sinks_from_one_scan(sample_index):
    """d_tally given: the clade counters and the plain counters are both right, and the pass scans what ONE plain tally pass
    scans -- mk_stats.scan_launches grows by exactly as much"""
    w, ix = sample_index
    G, ms, mi = w.s.c.G, 10, 60.0
    lib = ix._lib
    for layout, which, seqs in (("fine", "all", w.s.queries), ("masked", "few", w.s.reads[:FEW])):
        clade = w.lay[layout]
        n = cr.n_clades(clade)
        with Map(ix, clade) as m, DevBuf(ix, 40 * n) as buf, DevBuf(ix, 32 * G) as tbuf, Uploaded(ix, seqs) as qs:
            check(lib.mk_clade_tally_reset(ix._h, buf.p, n))
            check(lib.mk_tally_reset(ix._h, tbuf.p, G))
            check(lib.mk_qset_run_tally(ix._h, qs, ms, mi, tbuf.p, G))      # (the set is sketched and prepared by its first pass)
            check(lib.mk_sync(ix._h))
            a = scans(ix)
            check(lib.mk_qset_run_tally(ix._h, qs, ms, mi, tbuf.p, G))
            check(lib.mk_sync(ix._h))
            b = scans(ix)
            check(run(ix, qs, ms, mi, m, buf, n, tbuf, G))
            check(lib.mk_sync(ix._h))
            c = scans(ix)
            assert (b - a).sum() > 0 and ((c - b) == (b - a)).all()          # (which == "few": the slab schedule's launches)
            np.testing.assert_array_equal(read(ix, buf, n), w.want(layout, ms, mi, which))
            plain = np.zeros((G, 4), np.uint64)
            check(lib.mk_tally_read(ix._h, tbuf.p, G, plain.ctypes.data))
            np.testing.assert_array_equal(plain, 3 * w.plain(ms, mi, which))
            # a tally too small for the ids the context reports: refused as mk_qset_run_tally refuses it
            assert run(ix, qs, ms, mi, m, buf, n, tbuf, G - 1) == MK_ERR_ARG
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(read(ix, buf, n), w.want(layout, ms, mi, which))


def test_refusals_leave_the_counters_alone(hip, sample):
    from oracle import oracle as orc
    s = sample.s
    G = 200
    short = synth.genome_bases(9, 0, s.c.K)                                 # exactly k long: sketch_size 0
    o = orc.OracleMiekki(*s.c.par)
    o.insert_sequences(s.c.seqs[:G] + [short])
    assert o.sketch_size[G] == 0
    lists = cr.per_query(o, o.query_sequences(s.queries[:40]), 10, 10.0)
    clade = cr.from_cuts((0, 3, 64, 130, 200))
    want = cr.clade_tally(lists, clade + [None])
    assert want.shape == (4, 5) and want[:, 0].sum() > 40
    ix = s.a.build(hip, 0, G)
    lib = ix._lib
    try:
        marks = np.arange(5 * 6, dtype=np.uint64).reshape(6, 5)
        out = np.zeros_like(marks)

        def untouched(buf):
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(buf.download(np.zeros_like(marks)), marks)

        # maps that are none: refused on the host, nothing made
        st, m = make_map(ix, [0] * 100 + [2] * 50 + [1] * 50)
        assert st == MK_ERR_ARG and m.value is None and b"genome 150 " in lib.mk_last_error()
        st, m = make_map(ix, [5, None, 4] + [7] * (G - 3))                  # (a left-out genome in between hides nothing)
        assert st == MK_ERR_ARG and m.value is None and b"genome 2 " in lib.mk_last_error()
        st, m = make_map(ix, clade[:G - 1])
        assert st == MK_ERR_ARG and m.value is None
        st, m = make_map(ix, clade + [3])
        assert st == MK_ERR_ARG and m.value is None
        assert lib.mk_clade_map_create(ix._h, None, G, C.byref(m)) == MK_ERR_ARG
        numbers = cr.as_u32(clade)
        assert lib.mk_clade_map_create(ix._h, numbers.ctypes.data, G, None) == MK_ERR_ARG
        with DevBuf(ix, 40 * 6) as buf, Uploaded(ix, s.queries[:40]) as qs, Uploaded(ix, []) as none, Map(ix, clade) as m, \
                Map(ix, [None] * G) as nothing, FromIndex(ix, np.arange(G)) as own:
            buf.upload(marks)
            assert lib.mk_clade_map_size(m) == 4 and lib.mk_clade_map_size(nothing) == 0
            mi = C.c_double(10.0)
            assert lib.mk_qset_run_clade_tally(None, qs, 10, mi, m, buf.p, 6, None, 0) == MK_ERR_ARG
            assert lib.mk_qset_run_clade_tally(ix._h, None, 10, mi, m, buf.p, 6, None, 0) == MK_ERR_ARG
            assert lib.mk_qset_run_clade_tally(ix._h, qs, 10, mi, None, buf.p, 6, None, 0) == MK_ERR_ARG
            assert lib.mk_qset_run_clade_tally(ix._h, qs, 10, mi, m, None, 6, None, 0) == MK_ERR_ARG
            assert b"null argument" in lib.mk_last_error()
            assert lib.mk_clade_tally_reset(ix._h, None, 6) == MK_ERR_ARG
            assert lib.mk_clade_tally_read(ix._h, buf.p, 6, None) == MK_ERR_ARG
            assert lib.mk_clade_tally_read(ix._h, None, 6, out.ctypes.data) == MK_ERR_ARG
            assert run(ix, qs, 10, 10.0, m, buf, 3) == MK_ERR_ARG           # n_clades too small
            assert b"clades up to 3" in lib.mk_last_error()
            untouched(buf)
            assert run(ix, none, 10, 10.0, m, buf, 6) == MK_OK              # an empty set
            assert run(ix, qs, 10, 10.0, nothing, buf, 0) == MK_OK          # every genome left out: nothing to count
            assert run(ix, qs, 10, 10.0, nothing, buf, 6) == MK_OK
            untouched(buf)
            # in one call: the same refusals, `out` as it was
            ptrs, lens = (C.c_char_p * 2)(*s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in s.queries[:2]])
            arr = cr.as_u32(clade)
            assert lib.mk_query_clade_tally(ix._h, ptrs, lens, 2, 10, mi, arr.ctypes.data, 3, out.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_clade_tally(ix._h, ptrs, lens, 2, 10, mi, None, 4, out.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_clade_tally(ix._h, ptrs, lens, 2, 10, mi, arr.ctypes.data, 4, None) == MK_ERR_ARG
            assert lib.mk_query_clade_tally(ix._h, None, None, 2, 10, mi, arr.ctypes.data, 4, out.ctypes.data) == MK_ERR_ARG
            down = cr.as_u32(clade[::-1])
            assert lib.mk_query_clade_tally(ix._h, ptrs, lens, 2, 10, mi, down.ctypes.data, 4, out.ctypes.data) == MK_ERR_ARG
            assert not out.any()
            # a genome exactly k long has sketch_size 0: with min_score 0 its intersection is 0 / 0.  It came after the map
            # was made: the map leaves it out, the refusal is about the index
            ix.insert_sequences([short])
            assert run(ix, qs, 0, 10.0, m, buf, 6) == MK_ERR_UNSUPPORTED
            assert b"NaN" in lib.mk_last_error()
            arr1 = cr.as_u32(clade + [3])
            assert lib.mk_query_clade_tally(ix._h, ptrs, lens, 2, 0, mi, arr1.ctypes.data, 4, out.ctypes.data) == MK_ERR_UNSUPPORTED
            assert not out.any()
            untouched(buf)
            check(run(ix, qs, 10, 10.0, m, buf, 6))                         # ... and at min_score 10 the pass runs, the new genome ignored
            check(lib.mk_sync(ix._h))
            got = buf.download(out.copy()) - marks
            np.testing.assert_array_equal(got[:4], want)
            assert not got[4:].any()
            buf.upload(marks)
            ix.select(np.arange(G))                                         # the k-long genome goes; the map and `own` name what was there before
            assert run(ix, qs, 10, 10.0, m, buf, 6) == MK_ERR_STATE
            assert b"clade map" in lib.mk_last_error()
            with Map(ix, clade) as fresh:
                assert run(ix, own, 10, 10.0, fresh, buf, 6) == MK_ERR_STATE   # a stale set, a fresh map
                untouched(buf)
                check(run(ix, qs, 10, 10.0, fresh, buf, 6))                 # ... and an uploaded set runs with it
                check(lib.mk_sync(ix._h))
                np.testing.assert_array_equal((buf.download(out.copy()) - marks)[:4], want)
    finally:
        ix.close()


def test_genomes_appended_after_the_map_are_left_out(hip, sample):
    """a map over the first 600 genomes, then 501 more appended: the pass counts what a map with the new genomes left out
    counts -- the best hit is chosen among the first 600 -- and a fresh map over all of them counts them"""
    w = sample
    s = w.s
    G0, G, ms, mi = 600, s.c.G, 10, 10.0
    clade = w.lay["fine"]
    old = clade[:G0] + [None] * (G - G0)
    want = cr.clade_tally(w.per_query(ms, mi), old)
    full = w.want("fine", ms, mi)
    n = cr.n_clades(clade)
    assert (want[:cr.n_clades(old), 2] != full[:cr.n_clades(old), 2]).any()                  # (some best hits move)
    ix = s.a.build(hip, 0, G0)
    try:
        with Map(ix, clade[:G0]) as m, DevBuf(ix, 40 * n) as buf:
            for i in range(G0, G, 64):
                ix.insert_sequences(s.c.seqs[i:min(i + 64, G)])
            assert ix.index_size == G
            check(ix._lib.mk_clade_tally_reset(ix._h, buf.p, n))
            with Uploaded(ix, s.queries) as qs:
                check(run(ix, qs, ms, mi, m, buf, n))
                got = read(ix, buf, n)
                np.testing.assert_array_equal(got[:len(want)], want)
                assert not got[len(want):].any()
        np.testing.assert_array_equal(ix.clade_tally(s.queries, clade, ms, mi), full)
    finally:
        ix.close()


def test_reported_ids_do_not_shift_clade_numbers(hip, sample):
    """genome_id_base 1000: clade numbers are the caller's; the plain counters beside them are indexed by reported id"""
    w = sample
    s = w.s
    G, base, ms, mi = s.c.G, 1000, 10, 100.0
    clade = w.lay["masked"]
    n = cr.n_clades(clade)
    ix = s.a.build(hip, genome_id_base=base)
    try:
        np.testing.assert_array_equal(pieces(ix, [s.queries], ms, mi, clade), w.want("masked", ms, mi))
        np.testing.assert_array_equal(ix.clade_tally(s.queries, clade, ms, mi), w.want("masked", ms, mi))
        with Map(ix, clade) as m, DevBuf(ix, 40 * n) as buf, DevBuf(ix, 32 * (base + G)) as tbuf, Uploaded(ix, s.queries) as qs:
            check(ix._lib.mk_clade_tally_reset(ix._h, buf.p, n))
            check(ix._lib.mk_tally_reset(ix._h, tbuf.p, base + G))
            assert run(ix, qs, ms, mi, m, buf, n, tbuf, base + G - 1) == MK_ERR_ARG
            check(run(ix, qs, ms, mi, m, buf, n, tbuf, base + G))
            np.testing.assert_array_equal(read(ix, buf, n), w.want("masked", ms, mi))
            plain = np.zeros((base + G, 4), np.uint64)
            check(ix._lib.mk_tally_read(ix._h, tbuf.p, base + G, plain.ctypes.data))
            assert not plain[:base].any()
            np.testing.assert_array_equal(plain[base:], w.plain(ms, mi))
    finally:
        ix.close()


def test_python_takes_none_and_minus_one(sample_index):
    w, ix = sample_index
    clade = w.lay["masked"]
    want = w.want("masked", 10, 60.0)
    as_ints = np.array([-1 if c is None else c for c in clade], np.int64)
    np.testing.assert_array_equal(ix.clade_tally(w.s.queries, as_ints, 10, 60.0), want)
    assert ix.clade_tally(w.s.queries, [None] * len(clade)).shape == (0, 5)
    with pytest.raises(ValueError):
        ix.clade_tally(w.s.queries, clade[:-1])
    from miekki_amd import lib as L
    with pytest.raises(L.MiekkiHipError) as e:
        ix.clade_tally(w.s.queries, clade[::-1])
    assert e.value.status == MK_ERR_ARG


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        assert ix.clade_tally(reads, []).shape == (0, 5)
        marks = np.arange(20, dtype=np.uint64).reshape(4, 5)
        out = marks.copy()
        ptrs, lens = (C.c_char_p * 2)(*reads), (C.c_uint64 * 2)(*[len(r) for r in reads])
        assert ix._lib.mk_query_clade_tally(ix._h, ptrs, lens, 2, 10, C.c_double(10.0), None, 4, out.ctypes.data) == MK_OK
        np.testing.assert_array_equal(out, marks)
        m = C.c_void_p()
        assert ix._lib.mk_clade_map_create(ix._h, None, 0, C.byref(m)) == MK_OK and m.value
        assert ix._lib.mk_clade_map_size(m) == 0
        with DevBuf(ix, 160) as buf, Uploaded(ix, reads) as qs:
            buf.upload(marks)
            assert run(ix, qs, 10, 10.0, m, buf, 4) == MK_OK
            check(ix._lib.mk_sync(ix._h))
            np.testing.assert_array_equal(buf.download(np.zeros_like(marks)), marks)
        ix._lib.mk_clade_map_free(ix._h, m)
    finally:
        ix.close()
