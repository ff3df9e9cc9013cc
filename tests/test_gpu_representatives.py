"""mk_index_representatives / Miekki.representatives: greedy representative clustering of the indexed genomes in id order,
computed on the device, must be, element for element, what the plain greedy of tests/representatives_ref.py makes of the
ORACLE's query_sequence rows and filter_results' pass test.  Nothing here is compared with the device's own families or lists."""
import ctypes as C

import numpy as np
import pytest

import families_ref as fr
import representatives_ref as rr
import synth

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


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
    """fr.Collection (in its own or in reversed order), its oracle rows, the threshold taken from them, the model's answer"""

    def __init__(self, G, fp_bits, seed, reverse=False):
        self.c = c = fr.Collection(G, fp_bits, seed)
        self.a = a = fr.Answer(c.par, c.seqs[::-1] if reverse else c.seqs)
        inter = fr.intersections(a.rows, a.ss, a.gs)
        self.mi = c.threshold_between_chain_links(inter[::-1, ::-1] if reverse else inter)
        self.lists = a.lists(10, self.mi)
        self.want = rr.greedy(rr.links(self.lists))


@pytest.fixture(scope="module")
def planted():
    made = {}

    def get(fp_bits, reverse=False):
        if (fp_bits, reverse) not in made:
            made[fp_bits, reverse] = Planted(1101, 8, 310_000, reverse) if fp_bits == 8 else Planted(603, 16, 320_000, reverse)
        return made[fp_bits, reverse]
    return get


@pytest.fixture(scope="module")
def planted_index(hip, planted):
    p = planted(8)
    ix = p.a.build(hip)
    yield p, ix
    ix.close()


@pytest.mark.parametrize("name", ["messy", "rnd3", "w16", "h16z", "dups"])
def test_representatives_of_the_parity_cases(hip, answers, name):
    a = answers(name)
    if name == "dups":
        # on the oracle: at (400, 10.0) the 300 copies are one cluster around the smallest copy, the four others stand alone
        rep = rr.representatives(a, 400, 10.0)
        sizes = np.bincount(rep)
        assert len(a.seqs) == 304 and sizes.max() == 300 and (sizes == 1).sum() == 4 and (sizes > 0).sum() == 5
        copies = np.nonzero(rep == sizes.argmax())[0]
        assert sizes.argmax() == copies.min() and len({a.seqs[g] for g in copies}) == 1
    ix = a.build(hip)
    try:
        ix.reset_stats()
        got = ix.representatives()
        np.testing.assert_array_equal(got, rr.representatives(a))
        assert got.dtype == np.uint32 and got.shape == (len(a.seqs),)
        assert ix.stats()["filter_ms"] > 0                                              # rows + resolve + propagate
        np.testing.assert_array_equal(ix.representatives(1, 1.0), rr.representatives(a, 1, 1.0))
        np.testing.assert_array_equal(ix.representatives(400, 10.0), rr.representatives(a, 400, 10.0))
    finally:
        ix.close()


def test_planted_one_byte_fingerprints(planted_index):
    """1,101 genomes: two 1,024-genome score tiles, G no multiple of 8, resolved as 1,024 ids and 77 more with links across"""
    p, ix = planted_index
    np.testing.assert_array_equal(ix.representatives(10, p.mi), p.want)


def test_planted_one_byte_fingerprints_dense(planted_index):
    """the default thresholds: chance matches pass, six representatives for 1,101 genomes, every in-set row full of links"""
    p, ix = planted_index
    want = rr.representatives(p.a)
    assert (want == np.arange(p.c.G)).sum() == 6
    np.testing.assert_array_equal(ix.representatives(), want)


def test_planted_two_byte_fingerprints(hip, planted):
    """603 genomes past the 512-genome tile"""
    p = planted(16)
    ix = p.a.build(hip)
    try:
        np.testing.assert_array_equal(ix.representatives(10, p.mi), p.want)
    finally:
        ix.close()


def test_planted_in_reversed_order(hip, planted, monkeypatch):
    """the nested pair's one link points from the smaller id to the larger, several sets apart"""
    p = planted(8, reverse=True)
    lo, hi = sorted(p.c.G - 1 - g for g in p.c.nested)
    assert p.lists[lo, hi] and not p.lists[hi, lo] and p.want[hi] == lo
    ix = p.a.build(hip)
    try:
        np.testing.assert_array_equal(ix.representatives(10, p.mi), p.want)
        monkeypatch.setenv("MIEKKI_REP_SET_IDS", "64")                                  # (lo and hi in different sets)
        np.testing.assert_array_equal(ix.representatives(10, p.mi), p.want)
    finally:
        ix.close()


def test_the_answer_does_not_depend_on_the_cut(planted_index, monkeypatch):
    p, ix = planted_index
    dense = rr.representatives(p.a)
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "16")
    for per in ("64", "1000", None):
        if per is None:
            monkeypatch.delenv("MIEKKI_REP_SET_IDS")
        else:
            monkeypatch.setenv("MIEKKI_REP_SET_IDS", per)
        np.testing.assert_array_equal(ix.representatives(10, p.mi), p.want)
        np.testing.assert_array_equal(ix.representatives(), dense)


def test_consistency_with_select_and_families(hip, planted):
    p = planted(8)
    ix = p.a.build(hip)
    try:
        rep = ix.representatives(10, p.mi)
        np.testing.assert_array_equal(rep, p.want)
        labels = ix.families(10, p.mi)
        np.testing.assert_array_equal(labels[rep], labels)
        keep = np.nonzero(rep == np.arange(len(rep)))[0]
        ix.select(keep)
        assert ix.index_size == len(keep) < p.c.G
        np.testing.assert_array_equal(ix.representatives(10, p.mi), np.arange(len(keep)))   # no two representatives are linked
    finally:
        ix.close()


def test_cold_rows_raw_and_packed(hip, answers, monkeypatch):
    """part of messy's 4 MiB matrix in page-locked host memory, as it is and after compress_index"""
    a = answers("messy")
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = a.build(hip)
    try:
        np.testing.assert_array_equal(ix.representatives(), rr.representatives(a))
        ix.compress_index()
        np.testing.assert_array_equal(ix.representatives(), rr.representatives(a))
        np.testing.assert_array_equal(ix.representatives(12, 100.0), rr.representatives(a, 12, 100.0))
    finally:
        ix.close()


def test_genome_id_base(hip, planted):
    p = planted(8)
    lo, G = 550, p.c.G
    want = rr.representatives(p.a, 10, p.mi, lo, G)
    assert (want != np.arange(G - lo)).sum() >= 3                                       # (on the oracle: clusters inside the half)
    ix = p.a.build(hip, lo, G, genome_id_base=500)
    try:
        got = ix.representatives(10, p.mi)
        assert got.min() >= 500
        np.testing.assert_array_equal(got, want + 500)
    finally:
        ix.close()


def test_refusals_and_edges(hip, answers):
    a = answers("messy")
    ix = a.build(hip)
    lib = ix._lib
    try:
        G = ix.index_size
        out = np.full(G + 1, 7, np.uint32)
        assert lib.mk_index_representatives(ix._h, 10, C.c_double(1.0), None) == MK_ERR_ARG
        # a genome exactly k long has sketch_size 0: with min_score 0 its intersection is 0 / 0
        short = synth.genome_bases(9, 0, a.par[0])
        ix.insert_sequences([short])
        assert lib.mk_index_representatives(ix._h, 0, C.c_double(1.0), out.ctypes.data) == MK_ERR_UNSUPPORTED
        assert (out == 7).all()
        b = fr.Answer(a.par, a.seqs + [short])                                          # ... and the next valid call is right
        np.testing.assert_array_equal(ix.representatives(1, 1.0), rr.representatives(b, 1, 1.0))
        np.testing.assert_array_equal(ix.representatives(), rr.representatives(b))
        assert lib.mk_index_import_begin(ix._h, 0) == MK_OK                             # an empty index
        assert ix.index_size == 0
        assert lib.mk_index_representatives(ix._h, 10, C.c_double(1.0), out.ctypes.data) == MK_OK
        assert (out == 7).all()
        assert lib.mk_index_representatives(ix._h, 10, C.c_double(1.0), None) == MK_OK
        assert ix.representatives().shape == (0,)
    finally:
        ix.close()
