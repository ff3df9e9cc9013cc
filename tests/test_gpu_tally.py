"""mk_tally_reset / mk_qset_run_tally / mk_tally_read / mk_query_tally and Miekki.tally: the profile of a read set -- per
genome, the queries that list it, list it alone, have it as their best hit, and the matches of those -- summed on the device
must be, counter for counter, what a host sum makes of the ORACLE's filter_results (tests/tally_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import synth
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED, MK_ERR_STATE = 0, -1, -2, -5
THRESHOLDS = [(10, 10.0), (10, 60.0), (10, 100.0)]
FEW = 500                          # reads of a set below 512 queries: see slab_reads_check


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """a tr.Sample and the oracle's tallies of its queries, each computed once"""

    def __init__(self, *args, **kw):
        self.s = tr.Sample(*args, **kw)
        self.memo = {}

    def want(self, ms, mi, which="all"):
        if (ms, mi, which) not in self.memo:
            rows = {"all": self.s.rows, "few": self.s.read_rows[:FEW], "genomes": self.s.a.rows}[which]
            self.memo[ms, mi, which] = tr.tally(self.s.o, rows, ms, mi)
        return self.memo[ms, mi, which]


@pytest.fixture(scope="module")
def sample():
    return Wanted()


@pytest.fixture(scope="module")
def sample_index(hip, sample):
    ix = sample.s.a.build(hip)
    yield sample, ix
    ix.close()


class DevBuf:
    def __init__(self, ix, nbytes):
        self.ix, self.p = ix, C.c_void_p()
        check(ix._lib.mk_dev_alloc(ix._h, max(nbytes, 32), C.byref(self.p)))

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


def run(ix, qs, ms, mi, buf, n_ids):
    return ix._lib.mk_qset_run_tally(ix._h, qs, ms, float(mi), buf.p, n_ids)


def read(ix, buf, n_ids):
    out = np.full((n_ids, 4), 0xdead, np.uint64)
    check(ix._lib.mk_tally_read(ix._h, buf.p, n_ids, out.ctypes.data))
    return out


def pieces(ix, seqs, ms, mi, n_ids=None):
    """mk_dev_alloc, mk_tally_reset, mk_qset_upload, mk_qset_run_tally, mk_tally_read"""
    n_ids = ix._p.genome_id_base + ix.index_size if n_ids is None else n_ids
    with DevBuf(ix, 32 * n_ids) as buf:
        check(ix._lib.mk_tally_reset(ix._h, buf.p, n_ids))
        with Uploaded(ix, seqs) as qs:
            check(run(ix, qs, ms, mi, buf, n_ids))
        return read(ix, buf, n_ids)


def test_sample_preconditions_from_the_oracle_alone(sample):
    """what the sample was made for, on the oracle's rows alone"""
    s = sample.s
    assert len(s.queries) == 628
    seen = {}
    for ms, mi in THRESHOLDS:
        pq = tr.per_query(s.o, s.rows, ms, mi)
        n = np.array([len(l) for l, _ in pq])
        by_matches = sum(b is not None and b[1] != max(int(row[g]) for g in l) for (l, b), row in zip(pq, s.rows))
        seen[mi] = ((n == 0).sum(), (n == 1).sum(), (n > 1).sum(), n.max(), by_matches, len({b[0] for _, b in pq if b}))
        assert ties_for_best(s.o, s.rows, ms, mi) == 0                    # (the tie tests have their own cases)
    assert seen[10.0][0] == 0 and seen[10.0][3] > 512 and seen[10.0][4] >= 20      # lists beyond one step of any walk; best is not most matches
    assert seen[60.0][1] >= 5 and seen[60.0][2] >= 300
    assert seen[100.0][0] >= 5 and seen[100.0][1] >= 100 and seen[100.0][2] >= 100 and seen[100.0][4] >= 10 and seen[100.0][5] >= 100


@pytest.mark.parametrize("chunk", [None, "16"])
@pytest.mark.parametrize("ms,mi", THRESHOLDS)
def test_sample_like_the_oracle(sample_index, monkeypatch, ms, mi, chunk):
    """628 short, long and whole-genome queries -- a mixed set -- in one call and through the pieces, in the default chunks
    and in chunks of 16 queries"""
    w, ix = sample_index
    if chunk:
        monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", chunk)
    want = w.want(ms, mi)
    ix.reset_stats()
    got = ix.tally(w.s.queries, ms, mi)
    assert got.dtype == np.uint64 and got.shape == (w.s.c.G, 4)
    np.testing.assert_array_equal(got, want)
    assert ix.stats()["filter_ms"] > 0                                     # the tally launches
    np.testing.assert_array_equal(pieces(ix, w.s.queries, ms, mi), want)


def slab_reads_check(w, ix):
    """At -h 9 the whole matrix is one range of the slab schedule even at MIEKKI_SLAB_MIB=1 (512 rows x 1 KiB), so the range
    table is never chosen here whatever MIEKKI_SLAB_MIN_QUERIES says: a set of 512 short reads or more takes the plain
    schedule (u32 scores).  Partial counts are what a set BELOW 512 short reads leaves, its entry lists cut by count -- so
    the first 500 reads, in the default environment.  (The range table: test_agreement_with_the_lists_that_exist, -h 14.)"""
    before = ix.stats()["scan_slab_launches"]
    for ms, mi in ((10, 10.0), (10, 100.0)):
        np.testing.assert_array_equal(ix.tally(w.s.reads[:FEW], ms, mi), w.want(ms, mi, "few"))
    assert ix.stats()["scan_slab_launches"] > before


def test_partial_counts_one_byte_fingerprints(sample_index, monkeypatch):
    """short reads in the slab schedule: the walk over one-byte partial counts, in one chunk and in chunks of 16 reads"""
    slab_reads_check(*sample_index)
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "16")
    slab_reads_check(*sample_index)


def test_partial_counts_two_byte_fingerprints(hip):
    """603 genomes past the 512-genome tile, two-byte partial counts"""
    w = Wanted(603, 16, 320_000, whole=())
    assert w.want(10, 10.0, "few")[512:, 0].sum() > 0                      # (genomes of the second step of the walk are listed)
    ix = w.s.a.build(hip)
    try:
        slab_reads_check(w, ix)
    finally:
        ix.close()


def test_scores_of_a_set_from_the_index(sample_index):
    """every indexed genome as a query from its stored column: the dense kernel's u32 scores, no slab launch"""
    w, ix = sample_index
    G = w.s.c.G
    before = ix.stats()["scan_slab_launches"]
    with DevBuf(ix, 32 * G) as buf, FromIndex(ix, np.arange(G)) as qs:
        for ms, mi in ((10, 10.0), (10, 60.0)):
            check(ix._lib.mk_tally_reset(ix._h, buf.p, G))
            check(run(ix, qs, ms, mi, buf, G))
            got = read(ix, buf, G)
            np.testing.assert_array_equal(got, w.want(ms, mi, "genomes"))
            # the same from families_ref.Answer's rows, in numpy: listed is a column sum of its pass matrix
            lists = w.s.a.lists(ms, mi)
            np.testing.assert_array_equal(got[:, 0], lists.sum(0).astype(np.uint64))
            alone = lists.sum(1) == 1
            np.testing.assert_array_equal(got[:, 1], lists[alone].sum(0).astype(np.uint64))
            assert got[:, 2].sum() == lists.any(1).sum()
    assert ix.stats()["scan_slab_launches"] == before


def test_passes_accumulate(sample_index):
    w, ix = sample_index
    ms, mi = 10, 60.0
    want, G, q = w.want(ms, mi), w.s.c.G, w.s.queries
    with DevBuf(ix, 32 * G) as buf:
        check(ix._lib.mk_tally_reset(ix._h, buf.p, G))
        for part in (q[:300], q[300:]):                                    # the set in two halves
            with Uploaded(ix, part) as qs:
                check(run(ix, qs, ms, mi, buf, G))
        np.testing.assert_array_equal(read(ix, buf, G), want)
        with Uploaded(ix, q) as qs:
            check(run(ix, qs, ms, mi, buf, G))                             # the same queries again: twice the counters
            np.testing.assert_array_equal(read(ix, buf, G), 2 * want)
            check(ix._lib.mk_tally_reset(ix._h, buf.p, G))                 # a reset in between: once
            check(run(ix, qs, ms, mi, buf, G))
            np.testing.assert_array_equal(read(ix, buf, G), want)


def test_second_slice_of_mk_query_tally(sample_index):
    """2^18 + 5 reads, 64 distinct ones repeated: mk_query_tally takes them as two uploaded sets and the counters are the sum
    over both -- the oracle's tally of each distinct read times how often it occurs, in exact integers.  Thresholds chosen on
    the CPU for reads of 100 bases (85 k-mers): at (5, 5.0) the oracle lists between 5 and 36 genomes for each of the 64."""
    w, ix = sample_index
    ms, mi = 5, 5.0
    reads, queries, times = synth.two_slices(w.s.c.seqs, 21)
    assert len(queries) == (1 << 18) + 5 and sum(times) == len(queries) and set(times) == {4096, 4097}
    rows = w.s.o.query_sequences(reads)
    each = [tr.tally(w.s.o, rows[i:i + 1], ms, mi) for i in range(len(reads))]
    assert all(t[:, 0].sum() >= 5 for t in each) and (sum(each)[:, 0] > 0).sum() >= 500   # (on the oracle: nothing passes on zeros)
    want = sum(t * np.uint64(m) for t, m in zip(each, times))
    assert want.dtype == np.uint64
    np.testing.assert_array_equal(ix.tally(queries, ms, mi), want)


def test_reported_ids_index_the_counters(hip, sample):
    """genome_id_base 1000: the entries below stay as they were reset, the others are the genomes' in order"""
    s = sample.s
    G, base = s.c.G, 1000
    ms, mi = 10, 100.0
    ix = s.a.build(hip, genome_id_base=base)
    try:
        got = pieces(ix, s.queries, ms, mi)
        assert got.shape == (base + G, 4)
        assert not got[:base].any()
        np.testing.assert_array_equal(got[base:], sample.want(ms, mi))
        np.testing.assert_array_equal(ix.tally(s.queries, ms, mi), sample.want(ms, mi))      # by local genome
        # a context that reports an id at n_ids: refused before any launch
        n_ids = base + G - 1
        marks = np.arange(4 * n_ids, dtype=np.uint64).reshape(n_ids, 4)
        with DevBuf(ix, 32 * n_ids) as buf, Uploaded(ix, s.queries[:50]) as qs:
            buf.upload(marks)
            assert run(ix, qs, ms, mi, buf, n_ids) == MK_ERR_ARG
            check(ix._lib.mk_sync(ix._h))
            np.testing.assert_array_equal(buf.download(np.zeros_like(marks)), marks)
    finally:
        ix.close()


def ties_for_best(o, rows, ms, mi):
    """queries whose largest intersection several genomes share -- and the reference's choice among them, the largest id"""
    n = 0
    for row in rows:
        full = o.filter_results(row, o.index_size, ms, mi)
        if not full:
            continue
        top = max(h[3] for h in full)
        equal = [h[0] for h in full if h[3] == top]
        assert o.filter_results(row, 1, ms, mi)[0][0] == max(equal)
        n += len(equal) > 1
    return n


def test_ties_duplicate_genomes(hip):
    """three hundred copies of one genome: every copy is the best hit, the reference's heap of one keeps the last"""
    from oracle import oracle as orc
    case = synth.case_dups()
    seqs = case.genome_sequences()
    o = orc.OracleMiekki(case.k, case.h, case.fp_bits, case.b, case.threshold)
    o.insert_sequences(seqs)
    qs = [s for _, s in case.query_sequences()]
    rows = o.query_sequences(qs)
    mi = 0.5 * case.threshold
    assert ties_for_best(o, rows, 10, mi) >= 5
    want = tr.tally(o, rows, 10, mi)
    assert want[303, 2] >= 5 and want[:303, 2].sum() < want[303, 2]        # the largest id takes the ties
    ix = hip.Miekki(case.k, case.h, case.fp_bits, case.b, case.threshold)
    try:
        ix.insert_sequences(seqs)
        np.testing.assert_array_equal(ix.tally(qs), want)                   # (the default thresholds: 10, 0.5 * threshold)
        np.testing.assert_array_equal(pieces(ix, qs, 10, mi), want)
    finally:
        ix.close()


def test_ties_equal_sizes_poked(hip):
    """genomes of one size poked with equal sketch and genome sizes: equal scores are equal intersections"""
    from oracle import oracle as orc
    from miekki_amd import lib as L
    k, h, G = 21, 12, 160
    seqs = [synth.strain_device(g, 80, 500, 0, 30_000) for g in range(G)]
    o = orc.OracleMiekki(k, h, 8, 32, 20)
    o.insert_sequences(seqs)
    ss, gs = np.full(G, 3000, np.uint32), np.full(G, 30_000, np.uint64)
    o.poke_sizes(ss, gs)
    rng = np.random.default_rng(5)
    qs = []
    for _ in range(60):
        g = int(rng.integers(0, G))
        off = int(rng.integers(0, len(seqs[g]) - 700))
        qs.append(seqs[g][off:off + 700])
    rows = o.query_sequences(qs)
    assert ties_for_best(o, rows, 10, 10.0) >= 1
    ix = hip.Miekki(k, h, 8, 32, 20)
    try:
        ix.insert_sequences(seqs)
        L.check(ix._lib.mk_index_import_sizes(ix._h, gs.ctypes.data, ss.ctypes.data))
        np.testing.assert_array_equal(ix.tally(qs, 10, 10.0), tr.tally(o, rows, 10, 10.0))
    finally:
        ix.close()


def test_refusals_leave_the_counters_alone(hip, sample):
    from oracle import oracle as orc
    s = sample.s
    G = 200
    short = synth.genome_bases(9, 0, s.c.K)                                 # exactly k long: sketch_size 0
    o = orc.OracleMiekki(*s.c.par)
    o.insert_sequences(s.c.seqs[:G] + [short])
    assert o.sketch_size[G] == 0
    want = tr.tally(o, o.query_sequences(s.queries[:40]), 10, 10.0)
    assert want[:G, 0].sum() > 40 and not want[G].any()
    ix = s.a.build(hip, 0, G)
    lib = ix._lib
    try:
        marks = np.arange(4 * (G + 1), dtype=np.uint64).reshape(G + 1, 4)
        out = np.zeros_like(marks)
        with DevBuf(ix, 32 * (G + 1)) as buf, Uploaded(ix, s.queries[:40]) as qs, Uploaded(ix, []) as none, \
                FromIndex(ix, np.arange(G)) as own:
            buf.upload(marks)
            mi = C.c_double(10.0)
            assert lib.mk_qset_run_tally(None, qs, 10, mi, buf.p, G) == MK_ERR_ARG
            assert lib.mk_qset_run_tally(ix._h, None, 10, mi, buf.p, G) == MK_ERR_ARG
            assert lib.mk_qset_run_tally(ix._h, qs, 10, mi, None, G) == MK_ERR_ARG
            assert lib.mk_tally_reset(ix._h, None, G) == MK_ERR_ARG
            assert lib.mk_tally_read(ix._h, buf.p, G, None) == MK_ERR_ARG
            assert lib.mk_tally_read(ix._h, None, G, out.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_tally(ix._h, None, None, 3, 10, mi, out.ctypes.data) == MK_ERR_ARG
            assert lib.mk_query_tally(ix._h, None, None, 0, 10, mi, None) == MK_ERR_ARG
            assert run(ix, none, 10, 10.0, buf, G) == MK_OK                 # an empty set
            # a genome exactly k long has sketch_size 0: with min_score 0 its intersection is 0 / 0
            ix.insert_sequences([short])
            assert run(ix, qs, 0, 10.0, buf, G + 1) == MK_ERR_UNSUPPORTED
            assert b"NaN" in lib.mk_last_error()
            ptrs, lens = (C.c_char_p * 2)(*s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in s.queries[:2]])
            assert lib.mk_query_tally(ix._h, ptrs, lens, 2, 0, mi, out.ctypes.data) == MK_ERR_UNSUPPORTED
            assert not out.any()
            ix.select(np.arange(G))                                         # the k-long genome goes; `own` names what was there before
            assert run(ix, own, 10, 10.0, buf, G + 1) == MK_ERR_STATE
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(buf.download(out), marks)
            check(run(ix, qs, 10, 10.0, buf, G + 1))                        # ... and an uploaded set still runs
            got = buf.download(out) - marks
            np.testing.assert_array_equal(got, want)
    finally:
        ix.close()


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        assert ix.tally(reads).shape == (0, 4)
        marks = np.arange(16, dtype=np.uint64).reshape(4, 4)
        out = marks.copy()
        ptrs, lens = (C.c_char_p * 2)(*reads), (C.c_uint64 * 2)(*[len(r) for r in reads])
        assert ix._lib.mk_query_tally(ix._h, ptrs, lens, 2, 10, C.c_double(10.0), out.ctypes.data) == MK_OK
        assert ix._lib.mk_query_tally(ix._h, ptrs, lens, 2, 10, C.c_double(10.0), None) == MK_OK
        np.testing.assert_array_equal(out, marks)
        with DevBuf(ix, 128) as buf, Uploaded(ix, reads) as qs:
            buf.upload(marks)
            assert run(ix, qs, 10, 10.0, buf, 4) == MK_OK
            check(ix._lib.mk_sync(ix._h))
            np.testing.assert_array_equal(buf.download(np.zeros_like(marks)), marks)
    finally:
        ix.close()


def test_agreement_with_the_lists_that_exist(hip, monkeypatch):
    """no oracle: strain reads, whose lists are long -- the tally is the host's sum over query_list's lists and best hits.
    At -h 14 and MIEKKI_SLAB_MIB=1 the slab schedule has sixteen ranges: the partial counts of the range table."""
    monkeypatch.setenv("MIEKKI_SLAB_MIN_QUERIES", "1")
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "1")
    SP, ST, SL, PPM = 3, 48, 50_000, 3000
    G = SP * ST
    seqs = [synth.strain_device(g, ST, PPM, 0, SL) for g in range(G)]
    ix = hip.Miekki(31, 14, 8, 33, 200)
    try:
        for g0 in range(0, G, 48):
            ix.insert_sequences(seqs[g0:g0 + 48])
        rng = np.random.default_rng(11)
        reads = []
        for _ in range(300):
            g = int(rng.integers(0, G))
            off = int(rng.integers(0, SL - 1000))
            reads.append(seqs[g][off:off + 1000])
        full, _ = ix.query_list(reads, None)
        one, _ = ix.query_list(reads, 1)
        assert max(len(f) for f in full) >= ST
        want = np.zeros((G, 4), np.uint64)
        for f, o in zip(full, one):
            for hit in f:
                want[hit[0], 0] += 1
            if len(f) == 1:
                want[f[0][0], 1] += 1
            if o:
                want[o[0][0], 2] += 1
                want[o[0][0], 3] += o[0][1]
        before = ix.stats()["scan_slab_launches"]
        np.testing.assert_array_equal(ix.tally(reads), want)
        assert ix.stats()["scan_slab_launches"] > before
    finally:
        ix.close()
