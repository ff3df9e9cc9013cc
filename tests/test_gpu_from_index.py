"""mk_qset_from_index / mk_qset_from_columns / mk_index_export_genomes_device and Miekki.query_indexed: querying indexed
genomes from their stored columns must give what the oracle's query_sequence gives for their SEQUENCES
(tests/test_stored_column_is_the_query.py proves the premise on the oracle's side)."""
import ctypes as C

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
MK_ERR_ARG, MK_ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


class Ref:
    """a case's genomes, the oracle built with insert_sequences, and query_sequence of every genome's sequence (once)"""

    def __init__(self, case, seqs=None):
        from oracle import oracle as orc
        self.case = case
        self.seqs = case.genome_sequences() if seqs is None else seqs
        self.par = (case.k, case.h, case.fp_bits, case.b, case.threshold)
        self.o = orc.OracleMiekki(*self.par)
        self.o.insert_sequences(self.seqs)
        self.rows, self.active = self.answer(self.o)

    def answer(self, o):
        memo = {}
        for s in set(self.seqs):
            memo[s] = o.query_sequence(s)
        return np.stack([memo[s][0] for s in self.seqs]), np.array([memo[s][1] for s in self.seqs], np.uint32)

    def build(self, hip):
        ix = hip.Miekki(*self.par)
        for i in range(0, len(self.seqs), 64):
            ix.insert_sequences(self.seqs[i:i + 64])
        return ix


class Plain:
    def __init__(self, k, h, fp_bits, b, threshold):
        self.k, self.h, self.fp_bits, self.b, self.threshold = k, h, fp_bits, b, threshold


@pytest.fixture(scope="module")
def refs():
    made = {}

    def get(name):
        if name not in made:
            if name == "distinct16":                             # 150 different genomes, two-byte fingerprints: what `dups` cannot tell apart
                made[name] = Ref(Plain(15, 9, 16, 32, 10), [synth.genome_bases(77_000 + g, 0, 2000 + 7 * g) for g in range(150)])
            else:
                made[name] = Ref((synth.CASES.get(name) or synth.EXTRA_CASES[name])())
        return made[name]
    return get


class QSet:
    """a query set made from the index (or from columns), freed on exit"""

    def __init__(self, ix, ids=None, d_cols=None, n=None):
        self.ix, self.lib, self.h = ix, ix._lib, C.c_void_p()
        if d_cols is None:
            self.ids = np.ascontiguousarray(ids, np.uint32)
            self.n = len(self.ids)
            hip_check(self.lib.mk_qset_from_index(ix._h, self.ids.ctypes.data, self.n, C.byref(self.h)))
        else:
            self.n = n
            hip_check(self.lib.mk_qset_from_columns(ix._h, d_cols, n, C.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.lib.mk_qset_free(self.ix._h, self.h)

    def scores(self):
        G = self.ix.index_size
        out = np.zeros((self.n, G), np.uint32)
        with DevBuf(self.ix, out.nbytes) as d:
            hip_check(self.lib.mk_qset_scores(self.ix._h, self.h, 0, self.n, d.p))
            hip_check(self.lib.mk_sync(self.ix._h))
            d.download(out)
        return out

    def active(self):
        a = np.zeros(self.n, np.uint32)
        hip_check(self.lib.mk_qset_active(self.ix._h, self.h, a.ctypes.data))
        return a


def hip_check(st):
    from miekki_amd import lib as L
    L.check(st)


class DevBuf:
    def __init__(self, ix, nbytes):
        self.ix, self.p, self.n = ix, C.c_void_p(), nbytes
        hip_check(ix._lib.mk_dev_alloc(ix._h, max(nbytes, 16), C.byref(self.p)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ix._lib.mk_dev_free(self.ix._h, self.p)

    def download(self, arr):
        hip_check(self.ix._lib.mk_dev_download(self.ix._h, arr.ctypes.data, self.p, arr.nbytes))

    def upload(self, arr):
        hip_check(self.ix._lib.mk_dev_upload(self.ix._h, self.p, arr.ctypes.data, arr.nbytes))


def all_ids(ix):
    return np.arange(ix.index_size, dtype=np.uint32)


def same_hits(got, o, rows, nres, thr):
    """bit for bit: genome, matches, jaccard, intersection"""
    for q, row in enumerate(rows):
        want = o.filter_results(row, nres, 10, 0.5 * thr)
        assert [tuple(x) for x in got[q]] == want, q


@pytest.mark.parametrize("name", ["messy", "rnd0", "rnd3", "w16", "h16z"])
def test_scores_and_hits_of_every_indexed_genome(hip, refs, name):
    r = refs(name)
    ix = r.build(hip)
    try:
        ix.reset_stats()
        with QSet(ix, all_ids(ix)) as qs:
            np.testing.assert_array_equal(qs.scores(), r.rows)
            np.testing.assert_array_equal(qs.active(), r.o.sketch_size)
            np.testing.assert_array_equal(qs.active(), r.active)
        hip_check(ix._lib.mk_sync(ix._h))
        hits, active = ix.query_indexed()
        assert ix.stats()["sketch_ms"] > 0                      # the gather is the set's sketch step
        same_hits(hits, r.o, r.rows, 10, r.case.threshold)
        np.testing.assert_array_equal(active, r.active)
        # a genome meets itself whole: wherever it is among its own hits (h16z's full sketches have genome_size 0 -- active^2
        # wraps, Miekki.cpp:289, 306 -- so their intersection with themselves is 0 and they are not), it is with all of its sketch
        seen = 0
        for g, row in enumerate(hits):
            for x in row:
                if x.genome == g:
                    assert x.matches == r.o.sketch_size[g] and x.jaccard == 1.0
                    seen += 1
        assert seen > 0
    finally:
        ix.close()


def test_entrant_rows_and_compact_rows_of_a_set_from_the_index(hip, refs):
    """mk_qset_run, mk_qset_run_compact and mk_qset_invalidate on such a set"""
    from miekki_amd import lib as L
    r = refs("messy")
    ix = r.build(hip)
    try:
        n, cap, thr = len(r.seqs), 256, r.case.threshold
        with QSet(ix, all_ids(ix)) as qs, DevBuf(ix, n * 4) as d_count, DevBuf(ix, n * cap * 24) as d_cand, DevBuf(ix, n * (cap + 1) * 8) as d_rows:
            for again in range(2):
                hip_check(ix._lib.mk_qset_run(ix._h, qs.h, 10, 10, 0.5 * thr, cap, d_count.p, d_cand.p))
                hip_check(ix._lib.mk_qset_run_compact(ix._h, qs.h, 10, 10, 0.5 * thr, cap, d_rows.p))
                hip_check(ix._lib.mk_sync(ix._h))
                count = np.zeros(n, np.uint32); d_count.download(count)
                cand = (L.Hit * (n * cap))(); hip_check(ix._lib.mk_dev_download(ix._h, cand, d_cand.p, n * cap * 24))
                rows = np.zeros((n, cap + 1), np.uint64); d_rows.download(rows)
                for q in range(n):
                    want = r.o.filter_results(r.rows[q], 10, 10, 0.5 * thr)
                    out = (L.Hit * 10)()
                    m = ix._lib.mk_filter_candidates(C.byref(cand, q * cap * 24), int(count[q]), 10, out)
                    assert [(out[i].genome, out[i].matches, out[i].jaccard, out[i].intersection) for i in range(m)] == want
                    assert int(rows[q, 0]) == int(count[q])
                    assert [int(w) for w in rows[q, 1:1 + int(count[q])]] == [cand[q * cap + i].genome | cand[q * cap + i].matches << 32 for i in range(int(count[q]))]
                hip_check(ix._lib.mk_qset_invalidate(ix._h, qs.h))       # the second round gathers again
    finally:
        ix.close()


@pytest.fixture(scope="module")
def dups(hip, refs):
    r = refs("dups")
    ix = r.build(hip)
    yield r, ix
    ix.close()


def test_every_hit_of_a_tie_heavy_collection(dups):
    """304 genomes, 300 tied copies: the list path, the overflow replays, five dense blocks"""
    r, ix = dups
    G = len(r.seqs)
    assert G == 304
    hits, active = ix.query_indexed(nresults=None)
    same_hits(hits, r.o, r.rows, G, r.case.threshold)
    np.testing.assert_array_equal(active, r.active)
    hits10, _ = ix.query_indexed()
    same_hits(hits10, r.o, r.rows, 10, r.case.threshold)


def id_shapes(G):
    shapes = {f"first{n}": list(range(n)) for n in (1, 3, 5, 63, 64, 65)}                 # pad slots; one short of, exactly, one past a run of 64
    shapes["descending"] = list(range(G - 1, G - 71, -1))
    shapes["repeated"] = [5, 5, 7, G - 3, 5, 0, 0]
    shapes["unaligned_run"] = list(range(3, 3 + 64))                                        # the run starts at a non-multiple of 16
    shapes["unaligned_runs"] = list(range(41, 41 + 64)) + list(range(G - 9, G))             # ... and ends at the index's last genome
    shapes["run_then_scatter"] = list(range(16, 80)) + [G - 1, 3, 52, 2]
    return shapes


@pytest.mark.parametrize("shape", sorted(id_shapes(304)))
def test_id_shapes_on_the_tie_heavy_collection(dups, shape):
    r, ix = dups
    ids = np.array(id_shapes(304)[shape], np.uint32)
    with QSet(ix, ids) as qs:
        np.testing.assert_array_equal(qs.scores(), r.rows[ids])
        np.testing.assert_array_equal(qs.active(), r.active[ids])
    hits, active = ix.query_indexed(ids, nresults=None)
    same_hits(hits, r.o, r.rows[ids], 304, r.case.threshold)
    np.testing.assert_array_equal(active, r.active[ids])


def test_id_shapes_on_distinct_genomes_with_two_byte_fingerprints(hip, refs):
    """`dups` holds 300 equal columns: a slot that took its neighbour's column would not show there.  150 different
    genomes at W = 2 (a row's piece of 64 genomes is 128 bytes: nine 16-byte chunks when it starts unaligned)."""
    r = refs("distinct16")
    ix = r.build(hip)
    try:
        for shape, ids in sorted(id_shapes(150).items()):
            ids = np.array(ids, np.uint32)
            with QSet(ix, ids) as qs:
                np.testing.assert_array_equal(qs.scores(), r.rows[ids], err_msg=shape)
                np.testing.assert_array_equal(qs.active(), r.active[ids], err_msg=shape)
        hits, _ = ix.query_indexed()
        same_hits(hits, r.o, r.rows, 10, r.case.threshold)
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["messy", "w16"])
def test_sets_from_exported_columns(hip, refs, name):
    """mk_qset_from_columns fed by the device export and by the host export uploaded again: W = 1, and W = 2 (the dump's
    big-endian values)"""
    r = refs(name)
    ix = r.build(hip)
    try:
        G = ix.index_size
        ids = np.array(list(range(G - 1, -1, -1)) + [0], np.uint32)                        # (any order, one column twice)
        n, nbytes = len(ids), (1 << r.case.h) * len(ids) * ix.W
        host = np.zeros(nbytes, np.uint8)
        hip_check(ix._lib.mk_index_export_genomes(ix._h, ids.ctypes.data, n, host.ctypes.data))
        with DevBuf(ix, nbytes) as d_a, DevBuf(ix, nbytes) as d_b:
            hip_check(ix._lib.mk_index_export_genomes_device(ix._h, ids.ctypes.data, n, d_a.p))
            back = np.zeros(nbytes, np.uint8); d_a.download(back)
            np.testing.assert_array_equal(back, host)
            d_b.upload(host)
            for d in (d_a, d_b):
                with QSet(ix, d_cols=d.p, n=n) as qs:
                    np.testing.assert_array_equal(qs.scores(), r.rows[ids])
                    np.testing.assert_array_equal(qs.active(), r.active[ids])
                    hip_check(ix._lib.mk_qset_invalidate(ix._h, qs.h))
                    np.testing.assert_array_equal(qs.scores(), r.rows[ids])                # its own copy: nothing to gather again
        bad = np.array([G], np.uint32)
        with DevBuf(ix, nbytes) as d:
            assert ix._lib.mk_index_export_genomes_device(ix._h, bad.ctypes.data, 1, d.p) == MK_ERR_ARG
    finally:
        ix.close()


def test_cold_rows_raw_and_packed(hip, refs, monkeypatch):
    """part of messy's 4 MiB matrix in page-locked host memory: the gather reads those rows in place; a packed index is
    unpacked first, as for an export"""
    r = refs("messy")
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = r.build(hip)
    try:
        for packed in (False, True):
            if packed:
                ix.compress_index()
            with QSet(ix, all_ids(ix)) as qs:
                np.testing.assert_array_equal(qs.scores(), r.rows)
                np.testing.assert_array_equal(qs.active(), r.active)
            hits, _ = ix.query_indexed()
            same_hits(hits, r.o, r.rows, 10, r.case.threshold)
    finally:
        ix.close()


def test_a_set_follows_the_index_and_notices_when_its_genomes_are_gone(hip):
    r = Ref(synth.CASES["messy"]())                              # (its own oracle: this test appends to it)
    ix = r.build(hip)
    try:
        G = ix.index_size
        assert ix._lib.mk_qset_from_index(ix._h, np.array([G], np.uint32).ctypes.data, 1, C.byref(C.c_void_p())) == MK_ERR_ARG
        assert ix._lib.mk_qset_from_index(ix._h, np.array([0], np.uint32).ctypes.data, 0, C.byref(C.c_void_p())) == MK_ERR_ARG
        with QSet(ix, all_ids(ix)) as qs:
            np.testing.assert_array_equal(qs.scores(), r.rows)
            more = [synth.genome_bases(52, 100, 20_000), synth.genome_bases(4444, 0, 9000)]
            ix.insert_sequences(more)
            r.o.insert_sequences(more)
            rows, active = r.answer(r.o)
            got = qs.scores()                                    # gathered again: rows of G + 2 columns
            assert got.shape == (G, G + 2)
            np.testing.assert_array_equal(got, rows)
            np.testing.assert_array_equal(qs.active(), active)
            hip_check(ix._lib.mk_index_import_begin(ix._h, 0))
            with DevBuf(ix, 4096) as d:
                assert ix._lib.mk_qset_scores(ix._h, qs.h, 0, qs.n, d.p) == MK_ERR_STATE
                assert ix._lib.mk_qset_run_compact(ix._h, qs.h, 10, 10, 1.0, 16, d.p) == MK_ERR_STATE
            hl = C.c_void_p()
            assert ix._lib.mk_qset_run_list(ix._h, qs.h, 10, 10, 1.0, C.byref(hl)) == MK_ERR_STATE
    finally:
        ix.close()
