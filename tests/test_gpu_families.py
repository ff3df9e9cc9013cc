"""mk_link_reset / mk_qset_run_link / mk_link_merge / mk_link_labels / mk_index_families and Miekki.families: the families of
the indexed genomes -- connected components of "one lists the other" -- computed on the device must be, element for element,
what a host union-find makes of the ORACLE's query_sequence rows and filter_results' pass test (tests/families_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import families_ref as fr
import synth

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED, MK_ERR_STATE = 0, -1, -2, -5


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


@pytest.fixture(scope="module")
def answers():
    made = {}

    def get(name):
        if name not in made:
            case = (synth.CASES.get(name) or synth.EXTRA_CASES[name])()
            made[name] = fr.Answer((case.k, case.h, case.fp_bits, case.b, case.threshold), case.genome_sequences())
        return made[name]
    return get


class Planted:
    """fr.Collection, its oracle rows, the threshold taken from them, the labels they give -- and the proof, on the oracle's
    rows alone, that the collection holds what it was made for"""

    def __init__(self, G, fp_bits, seed):
        self.c = c = fr.Collection(G, fp_bits, seed)
        self.a = a = fr.Answer(c.par, c.seqs)
        inter = fr.intersections(a.rows, a.ss, a.gs)
        self.mi = c.threshold_between_chain_links(inter)
        lists = a.lists(10, self.mi)
        self.want = fr.family_labels(lists)
        off = lists & ~np.eye(G, dtype=bool)
        x, y, z = c.chain
        assert off[x, y] and off[y, z] and not off[x, z] and not off[z, x]               # a chain: joined only through its middle
        assert self.want[x] == self.want[z]
        assert (off & ~off.T).any()                                                       # listed in one direction only
        n0, n1 = c.nested
        assert off[n1, n0] and not off[n0, n1] and self.want[n0] == self.want[n1]
        sizes = np.bincount(self.want)
        assert (sizes == 1).sum() >= 2 and (sizes >= 3).sum() >= 2
        tile = 8192 // fp_bits
        for fam in (c.species_a, c.species_b, c.chain):                                   # families across tiles and sets of 64 ids
            assert len(set(self.want[fam])) == 1
            assert min(fam) < tile <= max(fam) and len({g // 64 for g in fam}) >= 3


@pytest.fixture(scope="module")
def planted():
    made = {}

    def get(fp_bits):
        if fp_bits not in made:
            made[fp_bits] = Planted(1101, 8, 310_000) if fp_bits == 8 else Planted(603, 16, 320_000)
        return made[fp_bits]
    return get


class DevBuf:
    def __init__(self, ix, nbytes):
        self.ix, self.p = ix, C.c_void_p()
        check(ix._lib.mk_dev_alloc(ix._h, max(nbytes, 16), C.byref(self.p)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ix._lib.mk_dev_free(self.ix._h, self.p)

    def download(self, arr):
        check(self.ix._lib.mk_dev_download(self.ix._h, arr.ctypes.data, self.p, arr.nbytes))
        return arr


def link(ix, qs, query_ids, min_score, mi, forest, n_ids):
    ids = np.ascontiguousarray(query_ids, np.uint32)
    return ix._lib.mk_qset_run_link(ix._h, qs, ids.ctypes.data, min_score, float(mi), forest.p, n_ids)


def labels_of(ix, forest, n_ids):
    out = np.full(n_ids, 0xffffffff, np.uint32)
    check(ix._lib.mk_link_labels(ix._h, forest.p, n_ids, out.ctypes.data))
    return out


def link_index(ix, forest, n_ids, min_score, mi, per=64):
    """every genome of the index, in sets of `per` ids, into the forest"""
    base = ix._p.genome_id_base
    for g0 in range(0, ix.index_size, per):
        ids = np.arange(base + g0, base + min(g0 + per, ix.index_size), dtype=np.uint32)
        qs = C.c_void_p()
        check(ix._lib.mk_qset_from_index(ix._h, ids.ctypes.data, len(ids), C.byref(qs)))
        try:
            check(link(ix, qs, ids, min_score, mi, forest, n_ids))
        finally:
            ix._lib.mk_qset_free(ix._h, qs)


@pytest.mark.parametrize("name", ["messy", "rnd3", "w16", "h16z", "dups"])
def test_families_of_the_parity_cases(hip, answers, name):
    a = answers(name)
    want = a.labels()
    if name == "dups":
        # every copy hammers one root; at the default thresholds the four strangers' chance matches (78-113 of 4,096 full
        # partitions in the oracle's rows) pass too, so min_score 400 keeps them out: exactly the 300 copies and four families of one
        assert len(a.seqs) == 304 and np.bincount(want).max() >= 300
        sizes = np.bincount(a.labels(400, 10.0))
        assert sizes.max() == 300 and (sizes == 1).sum() == 4
    ix = a.build(hip)
    try:
        ix.reset_stats()
        got = ix.families()
        np.testing.assert_array_equal(got, want)
        assert got.dtype == np.uint32
        assert ix.stats()["filter_ms"] > 0                                              # the link pass
        np.testing.assert_array_equal(ix.families(1, 1.0), a.labels(1, 1.0))             # other thresholds, other families
        np.testing.assert_array_equal(ix.families(400, 10.0), a.labels(400, 10.0))
    finally:
        ix.close()


@pytest.fixture(scope="module")
def planted_index(hip, planted):
    p = planted(8)
    ix = p.a.build(hip)
    yield p, ix
    ix.close()


def test_planted_families_one_byte_fingerprints(planted_index):
    """1,101 genomes: two 1,024-genome score tiles, G no multiple of 8, eighteen sets of 64 ids"""
    p, ix = planted_index
    np.testing.assert_array_equal(ix.families(10, p.mi), p.want)


def test_planted_families_over_several_sets_and_chunks(planted_index, monkeypatch):
    """mk_index_families' own loop over the index cut into eighteen sets of 64 ids (the last of 13: families reach across
    sets), each set scanned in chunks of 16 queries: the labels of the oracle's rows, and byte for byte the uncut answer"""
    p, ix = planted_index
    assert p.c.G == 1101 and -(-p.c.G // 64) == 18 and p.c.G % 64 == 13
    ix.reset_stats()
    whole = ix.families(10, p.mi)
    scans = ix.stats()["scan_launches"]                                     # (one set, one chunk)
    monkeypatch.setenv("MIEKKI_REP_SET_IDS", "64")
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "16")
    cut = ix.families(10, p.mi)
    assert ix.stats()["scan_launches"] == scans * (1 + 17 * 4 + 1)           # seventeen sets of four chunks and one of one
    np.testing.assert_array_equal(cut, p.want)
    assert cut.dtype == whole.dtype and cut.tobytes() == whole.tobytes()


def test_planted_families_two_byte_fingerprints(hip, planted):
    """603 genomes past the 512-genome tile"""
    p = planted(16)
    ix = p.a.build(hip)
    try:
        np.testing.assert_array_equal(ix.families(10, p.mi), p.want)
    finally:
        ix.close()


def test_linking_twice_and_in_other_sets_changes_nothing(planted_index):
    p, ix = planted_index
    G = p.c.G
    with DevBuf(ix, 4 * G) as forest:
        check(ix._lib.mk_link_reset(ix._h, forest.p, G))
        np.testing.assert_array_equal(labels_of(ix, forest, G), np.arange(G))
        link_index(ix, forest, G, 10, p.mi, per=64)
        np.testing.assert_array_equal(labels_of(ix, forest, G), p.want)
        link_index(ix, forest, G, 10, p.mi, per=1000)                                   # again, cut differently
        np.testing.assert_array_equal(labels_of(ix, forest, G), p.want)
        parent = forest.download(np.zeros(G, np.uint32))
        assert (parent <= np.arange(G)).all()                                           # the forest's invariant
        np.testing.assert_array_equal(p.want[parent], p.want)


@pytest.mark.parametrize("fp_bits", [8, 16])
def test_uploaded_queries_join_what_they_list(hip, planted, planted_index, fp_bits):
    """1 kb pieces of the genomes (the slab schedule: partial counts, one- and two-byte) and three queries beyond the short
    sketch (a mixed set: its second part takes the dense kernel's scores); piece q stands for id G + q"""
    p = planted(fp_bits)
    ix = planted_index[1] if fp_bits == 8 else p.a.build(hip)
    try:
        G, seqs = p.c.G, p.c.seqs
        src = sorted(set(p.c.species_a + p.c.species_b + p.c.chain + p.c.nested + list(range(0, G, 9))))
        pieces = [seqs[g][(37 * g) % 400:(37 * g) % 400 + 1000] for g in src]
        pieces += [seqs[5] + seqs[p.c.chain[1]], seqs[G - 2] + seqs[G - 3], seqs[p.c.species_a[1]] + seqs[77]]
        nq = len(pieces)
        rows = np.stack([p.a.o.query_sequence(s)[0] for s in pieces])
        for min_score, mi in ((40, 10.0), (10, p.mi / 3)):
            lists = p.a.lists(min_score, mi, rows)
            want = fr.family_labels(lists, np.arange(G, G + nq), G + nq)
            sizes = np.bincount(want)
            assert lists.sum(1).max() >= 3 and 2 < (sizes > 0).sum() < G and sizes.max() >= 5   # (on the oracle: something to join, not everything)
            ptrs, lens = (C.c_char_p * nq)(*pieces), (C.c_uint64 * nq)(*[len(s) for s in pieces])
            qs = C.c_void_p()
            check(ix._lib.mk_qset_upload(ix._h, ptrs, lens, nq, C.byref(qs)))
            try:
                ix.reset_stats()
                with DevBuf(ix, 4 * (G + nq)) as forest:
                    check(ix._lib.mk_link_reset(ix._h, forest.p, G + nq))
                    check(link(ix, qs, np.arange(G, G + nq), min_score, mi, forest, G + nq))
                    np.testing.assert_array_equal(labels_of(ix, forest, G + nq), want)
                assert ix.stats()["scan_slab_launches"] > 0
            finally:
                ix._lib.mk_qset_free(ix._h, qs)
    finally:
        if fp_bits != 8:
            ix.close()


def test_two_shard_forests_folded_into_one(hip, planted):
    """two contexts, each with half of the genomes and a forest over all ids; a run of ids is a set from the index on its
    owner and a set from the exported columns on the other; mk_link_merge folds the second forest into the first"""
    p = planted(8)
    G, half = p.c.G, 550
    shard = [p.a.build(hip, 0, half), p.a.build(hip, half, G, genome_id_base=half)]
    lib = shard[0]._lib
    try:
        nbytes_col = (1 << p.c.H) * 64
        with DevBuf(shard[0], 4 * G) as f0, DevBuf(shard[1], 4 * G) as f1, DevBuf(shard[0], 4 * G) as other, \
                DevBuf(shard[0], nbytes_col) as c0, DevBuf(shard[1], nbytes_col) as c1:
            forest, cols = [f0, f1], [c0, c1]
            for d in range(2):
                check(lib.mk_link_reset(shard[d]._h, forest[d].p, G))
            bounds = [0, half, G]
            for o in range(2):
                for g0 in range(bounds[o], bounds[o + 1], 64):
                    ids = np.arange(g0, min(g0 + 64, bounds[o + 1]), dtype=np.uint32)
                    n, sets = len(ids), [C.c_void_p(), C.c_void_p()]
                    check(lib.mk_qset_from_index(shard[o]._h, ids.ctypes.data, n, C.byref(sets[o])))
                    check(lib.mk_index_export_genomes_device(shard[o]._h, ids.ctypes.data, n, cols[o].p))
                    check(lib.mk_dev_copy(shard[1 - o]._h, cols[1 - o].p, shard[o]._h, cols[o].p, (1 << p.c.H) * n))
                    check(lib.mk_qset_from_columns(shard[1 - o]._h, cols[1 - o].p, n, C.byref(sets[1 - o])))
                    try:
                        for d in range(2):
                            check(link(shard[d], sets[d], ids, 10, p.mi, forest[d], G))
                    finally:
                        for d in range(2):
                            lib.mk_qset_free(shard[d]._h, sets[d])
            for d in range(2):                                                          # neither shard alone has the answer
                assert not np.array_equal(labels_of(shard[d], forest[d], G), p.want)
            check(lib.mk_dev_copy(shard[0]._h, other.p, shard[1]._h, f1.p, 4 * G))
            check(lib.mk_link_merge(shard[0]._h, f0.p, other.p, G))
            np.testing.assert_array_equal(labels_of(shard[0], f0, G), p.want)
    finally:
        for ix in shard:
            ix.close()


def test_cold_rows_raw_and_packed(hip, answers, monkeypatch):
    """part of messy's 4 MiB matrix in page-locked host memory, as it is and after compress_index"""
    a = answers("messy")
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = a.build(hip)
    try:
        np.testing.assert_array_equal(ix.families(), a.labels())
        ix.compress_index()
        np.testing.assert_array_equal(ix.families(), a.labels())
        np.testing.assert_array_equal(ix.families(12, 100.0), a.labels(12, 100.0))
    finally:
        ix.close()


def test_ids_beyond_the_forest_are_refused_before_any_launch(planted_index):
    p, ix = planted_index
    G, lib = p.c.G, ix._lib
    ids = np.arange(64, dtype=np.uint32)
    qs = C.c_void_p()
    check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, 64, C.byref(qs)))
    try:
        with DevBuf(ix, 4 * (G + 8)) as forest:
            check(lib.mk_link_reset(ix._h, forest.p, G + 8))
            bad = ids.copy(); bad[63] = G + 8                                           # a query id at n_ids
            assert link(ix, qs, bad, 10, p.mi, forest, G + 8) == MK_ERR_ARG
            assert link(ix, qs, ids, 10, p.mi, forest, G - 1) == MK_ERR_ARG           # a reported genome id at n_ids
            assert lib.mk_qset_run_link(ix._h, qs, None, 10, C.c_double(p.mi), forest.p, G) == MK_ERR_ARG
            assert lib.mk_qset_run_link(ix._h, qs, ids.ctypes.data, 10, C.c_double(p.mi), None, G) == MK_ERR_ARG
            assert lib.mk_qset_run_link(ix._h, None, ids.ctypes.data, 10, C.c_double(p.mi), forest.p, G) == MK_ERR_ARG
            check(lib.mk_sync(ix._h))
            np.testing.assert_array_equal(forest.download(np.zeros(G + 8, np.uint32)), np.arange(G + 8))   # untouched
            check(link(ix, qs, ids, 10, p.mi, forest, G + 8))                           # ... and the set still runs
            got = labels_of(ix, forest, G + 8)
            np.testing.assert_array_equal(got[:64], p.want[:64])
            np.testing.assert_array_equal(got[G:], np.arange(G, G + 8))
    finally:
        lib.mk_qset_free(ix._h, qs)


def test_stale_sets_nan_candidates_and_empty_indexes(hip, answers):
    a = answers("messy")
    ix = a.build(hip)
    lib = ix._lib
    try:
        G = ix.index_size
        ids = np.arange(G, dtype=np.uint32)
        qs = C.c_void_p()
        check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, G, C.byref(qs)))
        try:
            with DevBuf(ix, 4 * (G + 1)) as forest:
                check(lib.mk_link_reset(ix._h, forest.p, G + 1))
                # a genome exactly k long has sketch_size 0: with min_score 0 its intersection is 0 / 0
                ix.insert_sequences([synth.genome_bases(9, 0, a.par[0])])
                assert link(ix, qs, ids, 0, 1.0, forest, G + 1) == MK_ERR_UNSUPPORTED
                assert lib.mk_index_families(ix._h, 0, C.c_double(1.0), np.zeros(G + 1, np.uint32).ctypes.data) == MK_ERR_UNSUPPORTED
                check(link(ix, qs, ids, 1, 1.0, forest, G + 1))                         # (min_score 1: no such candidate)
                check(lib.mk_index_import_begin(ix._h, 0))                              # the ids name nothing now
                assert link(ix, qs, ids, 10, 1.0, forest, G + 1) == MK_ERR_STATE
        finally:
            lib.mk_qset_free(ix._h, qs)
        assert ix.index_size == 0
        untouched = np.full(4, 7, np.uint32)
        assert lib.mk_index_families(ix._h, 10, C.c_double(1.0), untouched.ctypes.data) == MK_OK
        assert (untouched == 7).all()
        assert lib.mk_index_families(ix._h, 10, C.c_double(1.0), None) == MK_OK
        assert ix.families().shape == (0,)
    finally:
        ix.close()
