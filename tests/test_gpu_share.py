"""mk_share_* / mk_qset_run_share / mk_query_abundance and Miekki.abundance: the pool of shared reads that the list walk fills
on the device must hold, counter for counter and list for list, what tests/share_ref.py makes of the ORACLE's filter_results --
three thresholds, three margins, over u32 scores and over one- and two-byte partial counts -- and the rounds over it must be,
bit for bit, share_ref's Python integers: abundances, last change, starved reads and shift."""
import ctypes as C

import numpy as np
import pytest

import clade_ref as cr
import lca_ref as lr
import share_ref as sr
import synth
import tally_ref as tr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED, MK_ERR_STATE = 0, -1, -2, -5
THRESHOLDS = [(10, 10.0), (10, 60.0), (10, 150.0)]
FEW = 500                          # a set below 512 short reads leaves partial counts, 512 or more u32 scores (test_gpu_lca.FEW)
G = 1101
AUTO = 0xffffffff


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


class Wanted:
    """an input (tally_ref.Sample or lca_ref.Grouped), the oracle's lists of its queries, the pools and the rounds, each once"""

    def __init__(self, s):
        self.s = s
        self.lists, self.pools, self.traces = {}, {}, {}

    def per_query(self, ms, mi, which="all"):
        if (ms, mi, which) not in self.lists:
            rows = {"all": self.s.rows, "few": self.s.read_rows[:FEW], "genomes": self.s.a.rows}[which]
            self.lists[ms, mi, which] = cr.per_query(self.s.o, rows, ms, mi)
        return self.lists[ms, mi, which]

    def pool(self, margin, ms, mi, which="all"):
        if (margin, ms, mi, which) not in self.pools:
            self.pools[margin, ms, mi, which] = sr.pool_of(self.per_query(ms, mi, which), margin, G)
        return self.pools[margin, ms, mi, which]

    def rounds(self, R, shift, margin, ms, mi, which="all"):
        """(A, delta, starved, shift) after R <= 25 rounds, from one run of 25"""
        key = (shift, margin, ms, mi, which)
        if key not in self.traces:
            trace = []
            s = sr.rounds(self.pool(margin, ms, mi, which), 25, shift, trace)[3]
            self.traces[key] = (trace, s)
        trace, s = self.traces[key]
        return trace[R - 1] + (s,)


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


class Pool:
    """mk_share_create ... mk_share_free"""

    def __init__(self, ix):
        self.ix, self.lib, self.p = ix, ix._lib, C.c_void_p()
        check(self.lib.mk_share_create(ix._h, C.byref(self.p)))
        self.G = ix.index_size

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.mk_share_free(self.ix._h, self.p)

    def run(self, qs, ms, mi, margin):
        return self.lib.mk_qset_run_share(self.ix._h, qs, ms, float(mi), margin, self.p)

    def run_seqs(self, seqs, ms, mi, margin, passes=1):
        with Uploaded(self.ix, seqs) as qs:
            for _ in range(passes):
                check(self.run(qs, ms, mi, margin))

    def add(self, off, ids):
        off, ids = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(ids, np.uint32)
        return self.lib.mk_share_add_lists(self.ix._h, self.p, off.ctypes.data, ids.ctypes.data, len(off) - 1)

    def add_pool(self, ref):
        check(self.add(*ref.offsets_ids()))

    def info(self):
        from miekki_amd import lib as L
        i = L.ShareInfo()
        check(self.lib.mk_share_info_read(self.ix._h, self.p, C.byref(i)))
        return {f[0]: int(getattr(i, f[0])) for f in L.ShareInfo._fields_}

    def export(self):
        """(info, unique, shared, the sorted multiset of lists)"""
        i = self.info()
        u, s = np.full(self.G, 0xdead, np.uint64), np.full(self.G, 0xdead, np.uint64)
        off, ids = np.full(i["shared_reads"] + 1, 0xdead, np.uint64), np.full(i["entries"], 0xdead, np.uint32)
        check(self.lib.mk_share_export(self.ix._h, self.p, u.ctypes.data, s.ctypes.data, off.ctypes.data, ids.ctypes.data))
        assert off[0] == 0 and off[-1] == i["entries"] and (np.diff(off.astype(np.int64)) >= 2).all()
        lists = sorted(tuple(int(g) for g in ids[int(off[r]):int(off[r + 1])]) for r in range(i["shared_reads"]))
        return i, u, s, lists

    def rounds(self, R, shift=AUTO):
        """(status, A, delta, starved, shift)"""
        from miekki_amd import lib as L
        a, res = np.full(self.G, 0xdead, np.uint64), L.ShareResult()
        st = self.lib.mk_share_rounds(self.ix._h, self.p, R, shift, a.ctypes.data, C.byref(res))
        assert st != MK_OK or res.rounds == R
        return st, a, int(res.delta), int(res.starved), int(res.shift)


def same_pool(got, ref):
    info, u, s, lists = got
    assert info == ref.info()
    np.testing.assert_array_equal(u, np.array(ref.unique, np.uint64))
    np.testing.assert_array_equal(s, np.array(ref.shared, np.uint64))
    assert lists == ref.multiset()


def same_rounds(got, want):
    st, a, delta, starved, shift = got
    check(st)
    np.testing.assert_array_equal(a, np.array(want[0], np.uint64))
    assert (delta, starved, shift) == tuple(want[1:])


# ---- the collector ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms,mi", THRESHOLDS)
@pytest.mark.parametrize("margin", sr.MARGINS)
@pytest.mark.parametrize("name", ["sample", "grouped"])
def test_pool_like_the_oracle(sample_index, grouped_index, name, margin, ms, mi):
    """the whole mixed set of 628 -- 620 short reads on u32 scores, eight whole genomes on the dense kernel's"""
    w, ix = sample_index if name == "sample" else grouped_index
    ref = w.pool(margin, ms, mi)
    ix.reset_stats()
    with Pool(ix) as p:
        p.run_seqs(w.s.queries, ms, mi, margin)
        same_pool(p.export(), ref)
    assert ix.stats()["filter_ms"] > 0                                      # the share launches


@pytest.mark.parametrize("margin", sr.MARGINS)
def test_one_byte_partial_counts(grouped_index, margin):
    """the first 500 reads: a set below 512 short reads is walked over one-byte partial counts"""
    w, ix = grouped_index
    before = ix.stats()["scan_slab_launches"]
    for ms, mi in THRESHOLDS:
        with Pool(ix) as p:
            p.run_seqs(w.s.reads[:FEW], ms, mi, margin)
            same_pool(p.export(), w.pool(margin, ms, mi, "few"))
    assert ix.stats()["scan_slab_launches"] > before                       # (partial counts were walked)


@pytest.mark.parametrize("margin", sr.MARGINS)
def test_two_byte_partial_counts(wide_index, margin):
    """16-bit fingerprints: 512 genomes per tile, the walk over two-byte partial counts; then the whole mixed set"""
    w, ix = wide_index
    before = ix.stats()["scan_slab_launches"]
    for ms, mi in THRESHOLDS:
        ref = w.pool(margin, ms, mi, "few")
        with Pool(ix) as p:
            p.run_seqs(w.s.reads[:FEW], ms, mi, margin)
            same_pool(p.export(), ref)
    assert ix.stats()["scan_slab_launches"] > before
    assert len(w.pool(100, 10, 60.0, "few").lists) > 0 and w.pool(10, 10, 60.0, "few").settled > 0
    with Pool(ix) as p:
        p.run_seqs(w.s.queries, 10, 60.0, margin)
        same_pool(p.export(), w.pool(margin, 10, 60.0))


def test_passes_accumulate_and_sets_leave_no_trace(grouped_index):
    w, ix = grouped_index
    q = w.s.queries
    for margin, ms, mi in ((10, 10, 10.0), (100, 10, 60.0), (0, 10, 150.0)):
        lists = w.per_query(ms, mi)
        with Pool(ix) as p:
            p.run_seqs(q, ms, mi, margin, passes=2)                         # two passes: the concatenation
            same_pool(p.export(), sr.pool_of(lists + lists, margin, G))
            check(p.lib.mk_share_reset(ix._h, p.p))
            assert p.info() == {"queries": 0, "assigned": 0, "shared_reads": 0, "entries": 0}
            for piece in (q[:211], q[211:500], q[500:]):                    # one set cut in three: the set
                p.run_seqs(piece, ms, mi, margin)
            same_pool(p.export(), w.pool(margin, ms, mi))


def test_sets_from_the_index(grouped_index):
    """every indexed genome as a query from its stored column, in sets of 64 ids: lists of whole species"""
    w, ix = grouped_index
    for margin in (10, 100):
        with Pool(ix) as p:
            for g0 in range(0, G, 64):
                with FromIndex(ix, np.arange(g0, min(G, g0 + 64))) as qs:
                    check(p.run(qs, 10, 10.0, margin))
            same_pool(p.export(), w.pool(margin, 10, 10.0, "genomes"))


@pytest.mark.parametrize("margin", (10, 100))
def test_chunks_of_sixteen_queries(grouped_index, monkeypatch, margin):
    """the chunks leave no trace: the pool grows chunk by chunk, every chunk's lists behind those before"""
    w, ix = grouped_index
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "16")
    with Pool(ix) as p:
        p.run_seqs(w.s.queries, 10, 10.0, margin)
        same_pool(p.export(), w.pool(margin, 10, 10.0))
    with Pool(ix) as p:
        p.run_seqs(w.s.reads[:FEW], 10, 10.0, margin)
        same_pool(p.export(), w.pool(margin, 10, 10.0, "few"))


# ---- the rounds ---------------------------------------------------------------------------------------------------------
# (margin, thresholds, which, starved reads of round 25 at shift 32: the issue's counts on the oracle's lists)
ROUNDS = [(100, (10, 10.0), "all", 8), (100, (10, 10.0), "few", 121), (100, (10, 60.0), "all", 6), (100, (10, 60.0), "few", 23),
          (10, (10, 10.0), "all", 3)]


@pytest.mark.parametrize("shift", [AUTO, 32])
@pytest.mark.parametrize("margin,at,which,starved", ROUNDS)
def test_rounds_like_the_reference(sample_index, margin, at, which, starved, shift):
    """collected on the device, then R = 1, 2, 25 over the same pool: A, delta, starved and shift are share_ref's"""
    w, ix = sample_index
    ms, mi = at
    with Pool(ix) as p:
        p.run_seqs(w.s.queries if which == "all" else w.s.reads[:FEW], ms, mi, margin)
        for R in (1, 2, 25):
            want = w.rounds(R, None if shift == AUTO else 32, margin, ms, mi, which)
            same_rounds(p.rounds(R, shift), want)
        assert want[2] == (starved if shift == 32 else 0)                   # (the starved path ran, or none was)
        if shift == 32:
            assert want[1] == 0                                             # delta = 0 after 25 rounds


LENGTHS = (2, 15, 16, 17, 63, 64, 65, 300, 1101)


def hand_made(n_lists=198, seed=11):
    """lists of the lengths at which the round kernel changes its path, interleaved so that short and long reads meet in one
    wave, between settled reads on a few genomes (so the weights differ) and unassigned ones"""
    rng = np.random.default_rng(seed)
    ref = sr.Pool(G)
    for i in range(n_lists):
        ref.add(sorted(rng.choice(G, LENGTHS[i % len(LENGTHS)], replace=False)))
        if i % 4 == 0:
            ref.add((int(rng.integers(0, 40)) * 27,))
        if i % 50 == 0:
            ref.add(())
    return ref


def in_pool_order(ref, rng):
    """the reference's queries as (offsets, ids) in a shuffled order: shared, settled and unassigned ones mixed"""
    all_lists = list(ref.lists) + [(g,) for g, n in enumerate(ref.unique) for _ in range(n)] + [()] * (ref.queries - ref.assigned)
    order = rng.permutation(len(all_lists))
    all_lists = [all_lists[i] for i in order]
    off = np.zeros(len(all_lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(l) for l in all_lists])
    return off, np.array([g for l in all_lists for g in l], np.uint32)


@pytest.mark.parametrize("team", [None, "8", "32", "64"])
def test_hand_made_lists(grouped_index, monkeypatch, team):
    """list lengths 2 ... 1,101 around every team width, through mk_share_add_lists; with MIEKKI_SHARE_TEAM the other
    mappings of reads to lanes give the same bits"""
    _, ix = grouped_index
    if team:
        monkeypatch.setenv("MIEKKI_SHARE_TEAM", team)
    ref = hand_made()
    assert {len(l) for l in ref.lists} == set(LENGTHS) and ref.settled and ref.queries > ref.assigned
    with Pool(ix) as p:
        check(p.add(*in_pool_order(ref, np.random.default_rng(2))))
        same_pool(p.export(), ref)
        for shift in (None, 32):
            trace = []
            s = sr.rounds(ref, 25 if team is None else 3, shift, trace)[3]
            for R in (1, 2, 25) if team is None else (1, 3):
                same_rounds(p.rounds(R, AUTO if shift is None else shift), trace[R - 1] + (s,))
            if team is None:
                assert shift is None or trace[-1][2] > 0                    # (reads starve at shift 32)
                same_rounds(p.rounds(25, AUTO if shift is None else shift), trace[-1] + (s,))   # run twice: the same answer


def test_bad_team_is_refused(grouped_index, monkeypatch):
    _, ix = grouped_index
    monkeypatch.setenv("MIEKKI_SHARE_TEAM", "12")
    with Pool(ix) as p:
        check(p.add([0, 2], [3, 5]))
        assert p.rounds(1)[0] == MK_ERR_ARG and b"MIEKKI_SHARE_TEAM" in ix._lib.mk_last_error()


def test_many_reads_on_two_genomes(grouped_index):
    """4,096 lists that all name the same two genomes: every add of a round lands on two words"""
    _, ix = grouped_index
    ref = sr.Pool(G)
    for _ in range(4096):
        ref.add((511, 512))
    for _ in range(3):
        ref.add((511,))
    ref.add((512,))
    with Pool(ix) as p:
        p.add_pool(ref)
        same_pool(p.export(), ref)
        for R, shift in ((1, None), (9, None), (9, 32), (9, 20)):
            same_rounds(p.rounds(R, AUTO if shift is None else shift), sr.rounds(ref, R, shift))


def test_settled_only_unassigned_only_and_nothing(grouped_index):
    _, ix = grouped_index
    with Pool(ix) as p:
        same_rounds(p.rounds(3), sr.rounds(sr.Pool(G), 3))                  # an empty pool: zeros, shift 0
        assert p.rounds(3, 32)[4] == 32
        ref = sr.Pool(G).add(()).add(()).add(())                            # only unassigned reads
        p.add_pool(ref)
        same_pool(p.export(), ref)
        got = p.rounds(2)
        same_rounds(got, sr.rounds(ref, 2))
        assert not got[1].any() and got[2:] == (0, 0, 0)
        for g in (0, 7, 7, 1100):                                           # only settled (and unassigned) reads
            ref.add((g,))
        check(p.add([0, 1, 2, 3, 4], [0, 7, 7, 1100]))
        same_pool(p.export(), ref)
        for R in (1, 2):
            same_rounds(p.rounds(R), sr.rounds(ref, R))
        assert p.rounds(2)[2] == 0 and int(p.rounds(1)[2]) == 4 << 32


def test_rounds_then_more_reads_then_rounds(sample_index):
    """the rounds leave the pool as it was: collected reads, rounds, hand-made lists behind them, rounds again"""
    w, ix = sample_index
    ref = sr.pool_of(w.per_query(10, 60.0), 10, G)
    with Pool(ix) as p:
        p.run_seqs(w.s.queries, 10, 60.0, 10)
        same_rounds(p.rounds(5), sr.rounds(ref, 5))
        same_pool(p.export(), ref)
        more = hand_made(27, seed=4)
        p.add_pool(more)
        for l in more.lists:
            ref.add(l)
        for g, n in enumerate(more.unique):
            for _ in range(n):
                ref.add((g,))
        for _ in range(more.queries - more.assigned):
            ref.add(())
        same_pool(p.export(), ref)
        same_rounds(p.rounds(5), sr.rounds(ref, 5))
        same_rounds(p.rounds(5, 32), sr.rounds(ref, 5, 32))


def test_python_and_the_one_call(sample_index):
    """Miekki.abundance -- mk_query_abundance, and with a shift the pieces -- against the same numbers"""
    w, ix = sample_index
    for margin, ms, mi, shift in ((10, 10, 10.0, None), (100, 10, 60.0, None), (10, 10, 10.0, 32), (0, 10, 150.0, None)):
        ref = w.pool(margin, ms, mi)
        a, u, s, info, res = ix.abundance(w.s.queries, 25, margin, ms, mi, shift)
        want = w.rounds(25, shift, margin, ms, mi)
        assert a.dtype == u.dtype == s.dtype == np.uint64 and a.shape == (G,)
        np.testing.assert_array_equal(a, np.array(want[0], np.uint64))
        np.testing.assert_array_equal(u, np.array(ref.unique, np.uint64))
        np.testing.assert_array_equal(s, np.array(ref.shared, np.uint64))
        assert info == ref.info()
        assert res == {"delta": want[1], "starved": want[2], "rounds": 25, "shift": want[3]}
    for bad in (101, -1, 2.5, "10", True):
        with pytest.raises(ValueError):
            ix.abundance(w.s.queries[:2], margin=bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            ix.abundance(w.s.queries[:2], rounds=bad)
    with pytest.raises(ValueError):
        ix.abundance(w.s.queries[:2], shift=33)
    a, u, s, info, res = ix.abundance([], 3)
    assert not a.any() and info == {"queries": 0, "assigned": 0, "shared_reads": 0, "entries": 0} and res["delta"] == 0


# ---- the error paths ------------------------------------------------------------------------------------------------------
def test_bad_lists_and_arguments_leave_the_pool_alone(grouped_index):
    w, ix = grouped_index
    lib = ix._lib
    ref = hand_made(20, seed=5)
    with Pool(ix) as p, Pool(ix) as other, Uploaded(ix, w.s.queries[:40]) as qs:
        p.add_pool(ref)
        for off, ids, says in (([0, 2, 4], [1, 2, 9, 9], b"list 1"),         # not strictly ascending
                               ([0, 2, 4], [1, 2, 9, 3], b"list 1"),
                               ([0, 1, 3], [4, 7, G], b"list 1"),            # beyond the index
                               ([0, 3, 2, 4], [1, 2, 3, 4], b"list 1"),      # an end before its beginning
                               ([0, 0, 0, 2], [5, 5], b"list 2")):
            assert p.add(off, ids) == MK_ERR_ARG and says in lib.mk_last_error(), (off, ids, lib.mk_last_error())
        same_pool(p.export(), ref)
        mi = C.c_double(10.0)
        assert lib.mk_qset_run_share(None, qs, 10, mi, 100, p.p) == MK_ERR_ARG
        assert lib.mk_qset_run_share(ix._h, None, 10, mi, 100, p.p) == MK_ERR_ARG
        assert lib.mk_qset_run_share(ix._h, qs, 10, mi, 100, None) == MK_ERR_ARG
        assert b"null argument" in lib.mk_last_error()
        assert p.run(qs, 10, 10.0, 101) == MK_ERR_ARG and b"margin" in lib.mk_last_error()
        assert lib.mk_share_add_lists(ix._h, p.p, None, None, 0) == MK_ERR_ARG
        assert lib.mk_share_create(ix._h, None) == MK_ERR_ARG
        assert lib.mk_share_info_read(ix._h, p.p, None) == MK_ERR_ARG
        from miekki_amd import lib as L
        res, a = L.ShareResult(), np.zeros(G, np.uint64)
        assert lib.mk_share_rounds(ix._h, p.p, 0, AUTO, a.ctypes.data, C.byref(res)) == MK_ERR_ARG       # no rounds
        assert lib.mk_share_rounds(ix._h, p.p, 1, AUTO, None, C.byref(res)) == MK_ERR_ARG
        assert lib.mk_share_rounds(ix._h, p.p, 1, AUTO, a.ctypes.data, None) == MK_ERR_ARG
        least = sr.auto_shift(ref)
        assert least >= 2
        assert p.rounds(1, least - 1)[0] == MK_ERR_ARG and b"shift" in lib.mk_last_error()
        assert p.rounds(1, 33)[0] == MK_ERR_ARG
        same_rounds(p.rounds(2, least), sr.rounds(ref, 2, least))
        same_pool(p.export(), ref)
        ptrs, lens = (C.c_char_p * 2)(*w.s.queries[:2]), (C.c_uint64 * 2)(*[len(q) for q in w.s.queries[:2]])
        assert lib.mk_query_abundance(ix._h, ptrs, lens, 2, 10, mi, 101, 5, a.ctypes.data, None, None, None, C.byref(res)) == MK_ERR_ARG
        assert lib.mk_query_abundance(ix._h, ptrs, lens, 2, 10, mi, 100, 0, a.ctypes.data, None, None, None, C.byref(res)) == MK_ERR_ARG
        assert lib.mk_query_abundance(ix._h, ptrs, lens, 2, 10, mi, 100, 5, None, None, None, None, C.byref(res)) == MK_ERR_ARG
        assert lib.mk_query_abundance(ix._h, ptrs, lens, 2, 10, mi, 100, 5, a.ctypes.data, None, None, None, None) == MK_ERR_ARG
        assert lib.mk_query_abundance(ix._h, None, None, 2, 10, mi, 100, 5, a.ctypes.data, None, None, None, C.byref(res)) == MK_ERR_ARG
        assert not a.any()
        assert other.info()["queries"] == 0


def test_stale_pools_and_sets(hip):
    from oracle import oracle as orc
    s = tr.Sample()
    n_g = 200
    short = synth.genome_bases(9, 0, s.c.K)                                 # exactly k long: sketch_size 0
    o = orc.OracleMiekki(*s.c.par)
    o.insert_sequences(s.c.seqs[:n_g])
    ref = sr.pool_of(cr.per_query(o, o.query_sequences(s.queries[:40]), 10, 10.0), 100, n_g)
    assert ref.assigned >= 40 and ref.lists
    ix = s.a.build(hip, 0, n_g)
    lib = ix._lib
    try:
        with Pool(ix) as p, Uploaded(ix, s.queries[:40]) as qs, FromIndex(ix, np.arange(n_g)) as own:
            check(p.run(qs, 10, 10.0, 100))
            same_pool(p.export(), ref)
            ix.insert_sequences([short])                                    # another G: the pool's counters have no word for the new genome
            assert p.run(qs, 10, 10.0, 100) == MK_ERR_STATE and b"share pool" in lib.mk_last_error()
            assert p.rounds(1)[0] == MK_ERR_STATE
            assert p.add([0, 1], [3]) == MK_ERR_STATE
            with Pool(ix) as fresh:
                # a genome exactly k long has sketch_size 0: with min_score 0 its intersection is 0 / 0
                assert fresh.run(qs, 0, 10.0, 100) == MK_ERR_UNSUPPORTED and b"NaN" in lib.mk_last_error()
                assert fresh.info()["queries"] == 0
                check(fresh.run(qs, 10, 10.0, 100))                         # ... and at min_score 10 the pass runs
                info, u, sh, lists = fresh.export()
                assert info == ref.info() and lists == ref.multiset() and not u[n_g] and not sh[n_g]
                ix.select(np.arange(n_g))                                   # the k-long genome goes: G as before, the ids' meaning is not
                assert fresh.run(qs, 10, 10.0, 100) == MK_ERR_STATE
            assert p.run(qs, 10, 10.0, 100) == MK_ERR_STATE                 # (made before the select, too)
            same_pool(p.export(), ref)                                      # ... and untouched by all of it
            with Pool(ix) as fresh:
                assert fresh.run(own, 10, 10.0, 100) == MK_ERR_STATE        # a stale set, a fresh pool
                assert fresh.info()["queries"] == 0
                check(fresh.run(qs, 10, 10.0, 100))
                same_pool(fresh.export(), ref)
                same_rounds(fresh.rounds(4), sr.rounds(ref, 4))
    finally:
        ix.close()


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        a, u, s, info, res = ix.abundance(reads, 3)
        assert a.shape == (0,) and info["assigned"] == 0 and res == {"delta": 0, "starved": 0, "rounds": 3, "shift": 0}
        with Pool(ix) as p, Uploaded(ix, reads) as qs:
            assert p.run(qs, 10, 10.0, 100) == MK_OK
            assert p.info() == {"queries": 2, "assigned": 0, "shared_reads": 0, "entries": 0}
            st, a, delta, starved, shift = p.rounds(2)
            assert (st, delta, starved, shift) == (MK_OK, 0, 0, 0)
    finally:
        ix.close()
