"""mk_qset_run_link_levels / mk_link_fold_levels / mk_index_hierarchy and Miekki.hierarchy: the nested families of the indexed
genomes at several thresholds from ONE all-vs-all pass must be, level by level and element for element, what a host union-find
makes of the ORACLE's rows at that level's thresholds (tests/families_ref.py) -- and what the existing one-level code gives."""
import ctypes as C

import numpy as np
import pytest

import families_ref as fr
import synth
import test_gpu_families as tf

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED, MK_ERR_STATE = 0, -1, -2, -5
check, DevBuf, labels_of = tf.check, tf.DevBuf, tf.labels_of

# families per level and (query, genome) pairs off the diagonal whose strictest passing level is that level, on the oracle
EXPECTED = {8: ((1, 1091, 1093, 1095, 1097), (858209, 13, 6, 4, 8)), 16: ((593, 593, 595, 598, 602), (7, 17, 6, 8, 2))}


class Nested:
    """tf.Planted with five levels around its threshold, the labels the oracle's rows give per level, and the proof -- on the
    oracle's rows alone -- that every forest is written directly and through the fold"""

    def __init__(self, fp_bits):
        self.p = p = tf.Planted(1101, 8, 310_000) if fp_bits == 8 else tf.Planted(603, 16, 320_000)
        self.c, self.a, self.G = p.c, p.a, p.c.G
        self.levels = [(10, 10.0), (10, p.mi), (300, p.mi), (330, 1600.0), (360, 1900.0)]
        assert all(x[0] <= y[0] and x[1] <= y[1] for x, y in zip(self.levels, self.levels[1:]))
        self.lists = [p.a.lists(s, mi) for s, mi in self.levels]
        self.want = np.stack([fr.family_labels(l) for l in self.lists])
        off = ~np.eye(self.G, dtype=bool)
        depth = np.sum(self.lists, axis=0) - 1                          # (nested lists: the strictest level a pair passes)
        for l in range(1, 5):
            assert not (self.lists[l] & ~self.lists[l - 1]).any()
        families = tuple(len(np.unique(w)) for w in self.want)
        pairs = tuple(int(((depth == l) & self.lists[0] & off).sum()) for l in range(5))
        assert (families, pairs) == EXPECTED[fp_bits], (families, pairs)
        one_way = self.lists[1] & ~self.lists[1].T & ~self.lists[2] & off
        assert one_way.sum() >= 3                                        # listed in one direction only, joined at level 1
        if fp_bits == 16:
            assert np.array_equal(self.want[0], self.want[1])            # a partition that repeats
        else:
            assert (self.want[0] == 0).all()                             # every wave hammers one root

    def level_array(self, levels=None):
        from miekki_amd import lib as L
        levels = self.levels if levels is None else levels
        return (L.Level * len(levels))(*[L.Level(int(s), 0, float(mi)) for s, mi in levels])


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


@pytest.fixture(scope="module")
def nested():
    made = {}

    def get(fp_bits):
        if fp_bits not in made:
            made[fp_bits] = Nested(fp_bits)
        return made[fp_bits]
    return get


@pytest.fixture(scope="module")
def indexes(hip, nested):
    made = {}

    def get(fp_bits):
        if fp_bits not in made:
            made[fp_bits] = nested(fp_bits).a.build(hip)
        return made[fp_bits]
    yield get
    for ix in made.values():
        ix.close()


@pytest.mark.parametrize("fp_bits", [8, 16])
def test_hierarchy_is_the_oracles_families_per_level(nested, indexes, fp_bits):
    n, ix = nested(fp_bits), indexes(fp_bits)
    ix.reset_stats()
    ix.families(*n.levels[0])
    one = ix.stats()["scan_launches"]
    ix.reset_stats()
    got = ix.hierarchy(n.levels)
    st = ix.stats()
    assert got.dtype == np.uint32 and got.shape == (5, n.G)
    np.testing.assert_array_equal(got, n.want)
    assert st["filter_ms"] > 0
    assert st["scan_launches"] == one                                    # one pass for five levels


@pytest.mark.parametrize("fp_bits", [8, 16])
def test_hierarchy_is_what_families_gives_level_by_level(nested, indexes, fp_bits):
    n, ix = nested(fp_bits), indexes(fp_bits)
    got = ix.hierarchy(n.levels)
    for l, lv in enumerate(n.levels):
        np.testing.assert_array_equal(got[l], ix.families(*lv))
        alone = ix.hierarchy([lv])
        assert alone.shape == (1, n.G)
        np.testing.assert_array_equal(alone[0], ix.families(*lv))


def test_hierarchy_over_several_sets_and_chunks(nested, indexes, monkeypatch):
    n, ix = nested(8), indexes(8)
    assert n.G == 1101 and -(-n.G // 64) == 18 and n.G % 64 == 13
    ix.reset_stats()
    whole = ix.hierarchy(n.levels)
    scans = ix.stats()["scan_launches"]                                   # (one set, one chunk)
    monkeypatch.setenv("MIEKKI_REP_SET_IDS", "64")
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "16")
    cut = ix.hierarchy(n.levels)
    assert ix.stats()["scan_launches"] == scans * (1 + 17 * 4 + 1)         # seventeen sets of four chunks and one of one
    np.testing.assert_array_equal(cut, n.want)
    assert cut.dtype == whole.dtype and cut.tobytes() == whole.tobytes()


def link_levels(ix, qs, query_ids, levels, n_levels, forests, n_ids):
    ids = np.ascontiguousarray(query_ids, np.uint32)
    return ix._lib.mk_qset_run_link_levels(ix._h, qs, ids.ctypes.data, levels, n_levels, forests.p, n_ids)


def reset_forests(ix, forests, n_levels, n_ids):
    for l in range(n_levels):
        check(ix._lib.mk_link_reset(ix._h, C.c_void_p(forests.p.value + 4 * l * n_ids), n_ids))


def forest_labels(ix, forests, l, n_ids):
    out = np.full(n_ids, 0xffffffff, np.uint32)
    check(ix._lib.mk_link_labels(ix._h, C.c_void_p(forests.p.value + 4 * l * n_ids), n_ids, out.ctypes.data))
    return out


def link_index_levels(ix, forests, n_ids, levels, per):
    base = ix._p.genome_id_base
    for g0 in range(0, ix.index_size, per):
        ids = np.arange(base + g0, base + min(g0 + per, ix.index_size), dtype=np.uint32)
        qs = C.c_void_p()
        check(ix._lib.mk_qset_from_index(ix._h, ids.ctypes.data, len(ids), C.byref(qs)))
        try:
            check(link_levels(ix, qs, ids, levels, len(levels), forests, n_ids))
        finally:
            ix._lib.mk_qset_free(ix._h, qs)


@pytest.mark.parametrize("fp_bits", [8, 16])
def test_raw_passes_accumulate_and_the_fold_is_idempotent(nested, indexes, fp_bits):
    n, ix = nested(fp_bits), indexes(fp_bits)
    G, lv = n.G, n.level_array()
    with DevBuf(ix, 4 * 5 * G) as forests:
        reset_forests(ix, forests, 5, G)
        link_index_levels(ix, forests, G, lv, per=64)
        np.testing.assert_array_equal(forest_labels(ix, forests, 4, G), n.want[4])       # the strictest level needs no fold
        link_index_levels(ix, forests, G, lv, per=1000)                                  # again, cut differently
        np.testing.assert_array_equal(forest_labels(ix, forests, 4, G), n.want[4])
        for _ in range(2):                                                               # fold, then fold again
            check(ix._lib.mk_link_fold_levels(ix._h, forests.p, G, 5))
            for l in range(5):
                np.testing.assert_array_equal(forest_labels(ix, forests, l, G), n.want[l])
        parent = forests.download(np.zeros(5 * G, np.uint32)).reshape(5, G)
        assert (parent <= np.arange(G)).all()                                            # the forests' invariant
        for l in range(5):
            np.testing.assert_array_equal(n.want[l][parent[l]], n.want[l])


@pytest.mark.parametrize("fp_bits", [8, 16])
def test_uploaded_queries_join_what_they_list_per_level(nested, indexes, fp_bits):
    """the 1 kb pieces and the three long queries of tf.test_uploaded_queries_join_what_they_list (slab partials of one and
    two bytes, dense scores in a mixed set); piece q stands for id G + q"""
    n, ix = nested(fp_bits), indexes(fp_bits)
    G, seqs, c = n.G, n.c.seqs, n.c
    src = sorted(set(c.species_a + c.species_b + c.chain + c.nested + list(range(0, G, 9))))
    pieces = [seqs[g][(37 * g) % 400:(37 * g) % 400 + 1000] for g in src]
    pieces += [seqs[5] + seqs[c.chain[1]], seqs[G - 2] + seqs[G - 3], seqs[c.species_a[1]] + seqs[77]]
    nq = len(pieces)
    rows = np.stack([n.a.o.query_sequence(s)[0] for s in pieces])
    levels = n.levels
    qids = np.arange(G, G + nq)
    want = [fr.family_labels(n.a.lists(s, mi, rows), qids, G + nq) for s, mi in levels]
    # (on the oracle: three different partitions, the two loosest join pieces with genomes; no piece has 300 matches anywhere)
    assert len({w.tobytes() for w in want}) == 3 and all(len(np.unique(w)) < G + nq for w in want[:2])
    assert all(len(np.unique(w)) == G + nq for w in want[2:])
    ptrs, lens = (C.c_char_p * nq)(*pieces), (C.c_uint64 * nq)(*[len(s) for s in pieces])
    qs = C.c_void_p()
    check(ix._lib.mk_qset_upload(ix._h, ptrs, lens, nq, C.byref(qs)))
    try:
        ix.reset_stats()
        with DevBuf(ix, 4 * 5 * (G + nq)) as forests:
            reset_forests(ix, forests, 5, G + nq)
            check(link_levels(ix, qs, qids, n.level_array(levels), 5, forests, G + nq))
            check(ix._lib.mk_link_fold_levels(ix._h, forests.p, G + nq, 5))
            for l in range(5):
                np.testing.assert_array_equal(forest_labels(ix, forests, l, G + nq), want[l])
        assert ix.stats()["scan_slab_launches"] > 0
    finally:
        ix._lib.mk_qset_free(ix._h, qs)


def test_genome_id_base(hip, nested):
    n = nested(16)
    lo = 500                                                  # genomes [500, 603): the second tile's relatives among them
    ix = n.a.build(hip, lo, n.G, genome_id_base=lo)
    try:
        got = ix.hierarchy(n.levels)
        assert got.shape == (5, n.G - lo)
        some = False
        for l, (s, mi) in enumerate(n.levels):
            lists = n.lists[l][lo:, lo:]
            want = fr.family_labels(lists) + lo                                          # reported ids
            np.testing.assert_array_equal(got[l], want)
            some |= bool((want != np.arange(lo, n.G)).any())
        assert some
        lv = n.level_array()
        ids = np.arange(lo, n.G, dtype=np.uint32)
        qs = C.c_void_p()
        check(ix._lib.mk_qset_from_index(ix._h, ids.ctypes.data, len(ids), C.byref(qs)))
        try:
            with DevBuf(ix, 4 * 5 * n.G) as forests:
                reset_forests(ix, forests, 5, n.G)
                check(link_levels(ix, qs, ids, lv, 5, forests, n.G))
                check(ix._lib.mk_link_fold_levels(ix._h, forests.p, n.G, 5))
                for l in range(5):
                    all_ids = forest_labels(ix, forests, l, n.G)
                    np.testing.assert_array_equal(all_ids[:lo], np.arange(lo))           # below the base: families of one
                    np.testing.assert_array_equal(all_ids[lo:], got[l])
        finally:
            ix._lib.mk_qset_free(ix._h, qs)
    finally:
        ix.close()


def test_refusals_come_before_any_launch(hip, nested, indexes):
    from miekki_amd import lib as L
    n, ix = nested(8), indexes(8)
    G, lib = n.G, ix._lib
    ids = np.arange(64, dtype=np.uint32)
    qs = C.c_void_p()
    check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, 64, C.byref(qs)))
    lv = n.level_array()
    nine = n.level_array([(10, 10.0)] * 9)
    try:
        with DevBuf(ix, 4 * 5 * (G + 8)) as forests:
            N = G + 8
            reset_forests(ix, forests, 5, N)

            def refused(status, word, *args):
                assert lib.mk_qset_run_link_levels(*args) == status
                assert word in lib.mk_last_error().decode(), lib.mk_last_error()
            good = [ix._h, qs, ids.ctypes.data, lv, 5, forests.p, N]
            for hole in (0, 1, 2, 3, 5):
                args = list(good); args[hole] = None
                refused(MK_ERR_ARG, "null", *args)
            for count in (0, 9):
                args = list(good); args[3], args[4] = nine, count
                refused(MK_ERR_ARG, "levels", *args)
            args = list(good); args[3] = n.level_array([(10, 10.0), (20, 10.0), (15, 10.0)]); args[4] = 3
            refused(MK_ERR_ARG, "level 2", *args)
            args = list(good); args[3] = n.level_array([(10, 10.0), (10, 5.0)]); args[4] = 2
            refused(MK_ERR_ARG, "level 1", *args)
            args = list(good); args[3] = n.level_array([(10, 10.0), (10, 20.0), (10, 30.0), (10, float("nan"))]); args[4] = 4
            refused(MK_ERR_ARG, "level 3", *args)
            bad = ids.copy(); bad[63] = N                                                # a query id at n_ids
            args = list(good); args[2] = bad.ctypes.data
            refused(MK_ERR_ARG, "beyond", *args)
            args = list(good); args[6] = G - 1                                           # a reported genome id at n_ids
            refused(MK_ERR_ARG, "beyond", *args)
            assert lib.mk_link_fold_levels(ix._h, None, N, 5) == MK_ERR_ARG
            assert lib.mk_link_fold_levels(ix._h, forests.p, N, 0) == MK_ERR_ARG
            assert lib.mk_link_fold_levels(ix._h, forests.p, N, 9) == MK_ERR_ARG
            out = np.full((5, G), 7, np.uint32)
            assert lib.mk_index_hierarchy(ix._h, nine, 9, out.ctypes.data) == MK_ERR_ARG
            assert lib.mk_index_hierarchy(ix._h, None, 5, out.ctypes.data) == MK_ERR_ARG
            assert lib.mk_index_hierarchy(ix._h, lv, 5, None) == MK_ERR_ARG
            assert (out == 7).all()
            with pytest.raises(L.MiekkiHipError):
                ix.hierarchy([(10, 10.0), (5, 10.0)])
            check(lib.mk_sync(ix._h))
            want = np.tile(np.arange(N, dtype=np.uint32), 5)
            np.testing.assert_array_equal(forests.download(np.zeros(5 * N, np.uint32)), want)   # untouched
            check(lib.mk_qset_run_link_levels(*good))                                    # ... and the set still runs
            check(lib.mk_link_fold_levels(ix._h, forests.p, N, 5))
            got = forest_labels(ix, forests, 1, N)
            np.testing.assert_array_equal(got[G:], np.arange(G, N))
    finally:
        lib.mk_qset_free(ix._h, qs)


def test_nan_candidates_stale_sets_and_empty_indexes(hip):
    case = synth.CASES["messy"]()
    a = fr.Answer((case.k, case.h, case.fp_bits, case.b, case.threshold), case.genome_sequences())
    ix = a.build(hip)
    lib = ix._lib
    from miekki_amd import lib as L
    try:
        G = ix.index_size
        N = G + 1
        ids = np.arange(G, dtype=np.uint32)
        zero = (L.Level * 2)(L.Level(0, 0, 1.0), L.Level(5, 0, 1.0))
        ok = (L.Level * 2)(L.Level(1, 0, 1.0), L.Level(5, 0, 1.0))
        qs = C.c_void_p()
        check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, G, C.byref(qs)))
        try:
            with DevBuf(ix, 4 * 2 * N) as forests:
                reset_forests(ix, forests, 2, N)
                ix.insert_sequences([synth.genome_bases(9, 0, a.par[0])])               # sketch_size 0
                assert lib.mk_qset_run_link_levels(ix._h, qs, ids.ctypes.data, zero, 2, forests.p, N) == MK_ERR_UNSUPPORTED
                assert lib.mk_last_error()
                assert lib.mk_index_hierarchy(ix._h, zero, 2, np.zeros(2 * N, np.uint32).ctypes.data) == MK_ERR_UNSUPPORTED
                check(lib.mk_sync(ix._h))
                np.testing.assert_array_equal(forests.download(np.zeros(2 * N, np.uint32)), np.tile(np.arange(N, dtype=np.uint32), 2))
                check(lib.mk_qset_run_link_levels(ix._h, qs, ids.ctypes.data, ok, 2, forests.p, N))
                check(lib.mk_index_import_begin(ix._h, 0))                               # the ids name nothing now
                assert lib.mk_qset_run_link_levels(ix._h, qs, ids.ctypes.data, ok, 2, forests.p, N) == MK_ERR_STATE
                assert lib.mk_last_error()
        finally:
            lib.mk_qset_free(ix._h, qs)
        assert ix.index_size == 0
        untouched = np.full(8, 7, np.uint32)
        assert lib.mk_index_hierarchy(ix._h, ok, 2, untouched.ctypes.data) == MK_OK
        assert (untouched == 7).all()
        assert lib.mk_index_hierarchy(ix._h, ok, 2, None) == MK_OK
        assert ix.hierarchy([(10, 1.0), (20, 2.0)]).shape == (2, 0)
    finally:
        ix.close()
