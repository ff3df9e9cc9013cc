"""mk_index_select / Miekki.select: keep the genomes ids[0 .. n) of an index, in that order, in place.

The reference has no such member, so the yardstick is the stream its loading constructor reads (Miekki.cpp:649-719): the
same genomes are built in the oracle, and numpy assembles the file that holds exactly the kept columns, the kept sizes and
the OLD Bloom filter.  The index's serialize() after select(ids) must be that stream byte for byte, and every query must
answer what OracleMiekki.deserialize(that stream) answers, bit for bit -- for a kept genome's sequence and for a removed
one's, whose partitions stay active through the old filter."""
import ctypes as C
import struct

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
MK_ERR_ARG, MK_ERR_STATE = -1, -5
K, B, THR = 21, 32, 10


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


class Coll:
    """distinct genomes (every fourth shares its first half with the one before it, so that queries hit more than
    themselves), the oracle built from them once, and its columns / sizes / Bloom bytes"""

    def __init__(self, name, G, fp_bits, h, length):
        from oracle import oracle as orc
        self.name, self.G, self.fp_bits, self.h, self.W = name, G, fp_bits, h, fp_bits // 8
        self.par = (K, h, fp_bits, B, THR)
        self.seqs = []
        for g in range(G):
            s = synth.genome_bases(910_000 + 7 * G + g, 0, length + 3 * (g % 37))
            if g % 4 == 3:
                s = self.seqs[-1][:length // 2] + s[length // 2:]
            self.seqs.append(s)
        assert len(set(self.seqs)) == G
        self.extra = [synth.genome_bases(990_000 + g, 0, length) for g in range(2)]      # appended after a select
        self.o = orc.OracleMiekki(*self.par)
        self.o.insert_sequences(self.seqs)
        self.cols = self.o.columns().reshape(1 << h, G, self.W).copy()
        self.ss, self.gs = self.o.sketch_size, self.o.genome_size
        self.bloom = self.o.bloom.copy()

    def stream(self, ids):
        """what dump_disk would write for an index of exactly the genomes `ids` under the collection's Bloom filter"""
        ids = np.asarray(ids, np.int64)
        hdr = struct.pack("<6IQBBIB", K, self.h, self.fp_bits, 5, len(ids), B, 1 << B, 0, 0, THR, 1)
        return np.concatenate([np.frombuffer(hdr, np.uint8), np.ascontiguousarray(self.cols[:, ids, :]).reshape(-1),
                               self.gs[ids].astype(np.uint64).view(np.uint8), self.bloom,
                               self.ss[ids].astype(np.uint32).view(np.uint8)])

    def build(self, hip):
        ix = hip.Miekki(*self.par)
        for i in range(0, self.G, 64):
            ix.insert_sequences(self.seqs[i:i + 64])
        return ix


SHAPES = {"A": (1100, 8, 10, 2000),      # crosses the 1,024-genome tile; pitch of two tiles
          "B": (600, 16, 10, 2000),      # crosses the 512-genome tile at two bytes
          "C": (150, 8, 9, 2000)}        # less than one tile


@pytest.fixture(scope="module")
def colls():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Coll(name, *SHAPES[name])
        return made[name]
    return get


def id_lists(name):
    G = SHAPES[name][0]
    rng = np.random.default_rng(20_000 + G)
    tile = 1024 if SHAPES[name][1] == 8 else 512
    lists = {
        "identity": list(range(G)),
        "reversal": list(range(G))[::-1],
        "permutation": rng.permutation(G).tolist(),
        "drop_first": list(range(1, G)),
        "drop_last": list(range(G - 1)),
        "last_only": [G - 1],
        "drop_each_third": [g for g in range(G) if g % 3 != 2],
        "random_subset": rng.permutation(G)[:G * 2 // 3].tolist(),
    }
    if G >= 41 + 700 + 1:
        lists["run_plus_scattered"] = list(range(41, 41 + 700)) + [G - 1, 3, 17]
    if G > tile:
        for n in (tile - 1, tile, tile + 1):
            lists[f"ascending_{n}"] = sorted(rng.permutation(G)[:n].tolist())
    return lists


CASES = [(name, key) for name in SHAPES for key in id_lists(name)]


def stream_equals(ix, want):
    """ix.serialize() == want, byte 32 masked as tests/test_gpu_edges.py does, piece by piece"""
    want = want.copy()
    want[32] = 0
    off = 0
    for piece in ix.serialize():
        got = np.frombuffer(piece, np.uint8)
        if off <= 32 < off + len(got):
            got = got.copy()
            got[32 - off] = 0
        assert off + len(got) <= len(want), "stream too long"
        if not np.array_equal(got, want[off:off + len(got)]):
            bad = int(np.flatnonzero(got != want[off:off + len(got)])[0]) + off
            raise AssertionError(f"stream differs at byte {bad}")
        off += len(got)
    assert off == len(want), (off, len(want))


def same_hits(got, o, rows, nres):
    """bit for bit: genome, matches, jaccard, intersection"""
    for q, row in enumerate(rows):
        assert [tuple(x) for x in got[q]] == o.filter_results(row, nres, 10, 0.5 * THR), q


def queries_equal(ix, c, ids, o2):
    """query_sequences, query, query_list and query_indexed against the oracle that loaded the expected stream"""
    n = len(ids)
    removed = sorted(set(range(c.G)) - set(ids))
    qs = [c.seqs[ids[0]], c.seqs[ids[-1]][100:1500], c.seqs[ids[n // 2]]]
    qs += [c.seqs[g] for g in (removed[:1] + removed[-1:])]          # active through the old filter, match nothing of their own
    rows = o2.query_sequences(qs)
    np.testing.assert_array_equal(ix.query_sequences(qs), rows)
    hits, act = ix.query(qs, 10, 10, 0.5 * THR)
    same_hits(hits, o2, rows, 10)
    assert [int(a) for a in act] == [o2.query_sequence(s)[1] for s in qs]
    hits, _ = ix.query_list(qs, None, 10, 0.5 * THR)
    same_hits(hits, o2, rows, n)
    some = sorted(set(list(range(min(n, 70))) + list(range(max(0, n - 6), n))))
    for nres in (10, None):
        hits, act = ix.query_indexed(some, nres, 10, 0.5 * THR)
        same_hits(hits, o2, np.stack([o2.query_sequence(c.seqs[ids[j]])[0] for j in some]), nres or n)
        np.testing.assert_array_equal(act, c.ss[[ids[j] for j in some]])


@pytest.mark.parametrize("name,key", CASES)
def test_select_gives_the_stream_of_the_kept_columns(hip, colls, name, key):
    from oracle import oracle as orc
    c = colls(name)
    ids = id_lists(name)[key]
    ix = c.build(hip)
    try:
        ix.file_names = [f"g{g}" for g in range(c.G)]
        ix.select(ids)
        assert ix.index_size == len(ids)
        np.testing.assert_array_equal(ix.sketch_size, c.ss[ids])
        np.testing.assert_array_equal(ix.genome_size, c.gs[ids])
        assert ix.file_names == [f"g{g}" for g in ids]
        want = c.stream(ids)
        stream_equals(ix, want)
        queries_equal(ix, c, ids, orc.OracleMiekki.deserialize(want))
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["C", "B"])
def test_a_second_select_composes(hip, colls, name):
    c = colls(name)
    rng = np.random.default_rng(5)
    first = rng.permutation(c.G)[:c.G - 20]
    second = rng.permutation(len(first))[:len(first) - 30]
    ix = c.build(hip)
    try:
        ix.select(first)
        ix.select(second)
        stream_equals(ix, c.stream(first[second]))
    finally:
        ix.close()


@pytest.mark.parametrize("name,key", [("C", "drop_each_third"), ("B", "random_subset"), ("A", "drop_first")])
def test_append_after_select_equals_append_after_loading_the_stream(hip, colls, tmp_path, name, key):
    """a dirty tail or stale sizes would show here: the load path is existing, trusted code"""
    c = colls(name)
    ids = id_lists(name)[key]
    (tmp_path / "want.idx").write_bytes(c.stream(ids).tobytes())
    ix = c.build(hip)
    back = hip.Miekki.load(str(tmp_path / "want.idx"))
    try:
        ix.select(ids)
        ix.insert_sequences(c.extra)
        back.insert_sequences(c.extra)
        assert ix.index_size == len(ids) + 2
        np.testing.assert_array_equal(ix.sketch_size, back.sketch_size)
        np.testing.assert_array_equal(ix.genome_size, back.genome_size)
        off = 0
        for a, b in zip(ix.serialize(), back.serialize()):
            assert a == b, f"streams differ in the piece at byte {off}"
            off += len(a)
    finally:
        ix.close(); back.close()


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("name,key", [("A", "permutation"), ("A", "drop_each_third"), ("B", "reversal")])
def test_select_with_cold_rows(hip, colls, monkeypatch, name, key, packed):
    """half of the matrix in page-locked host memory, raw and packed: the same streams"""
    from oracle import oracle as orc
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")               # (read when the context is made) 1,024 rows x 2 KiB: 512 stay in HBM
    c = colls(name)
    ids = id_lists(name)[key]
    ix = c.build(hip)
    try:
        if packed:
            ix.compress_index()
        ix.select(ids)
        want = c.stream(ids)
        stream_equals(ix, want)
        queries_equal(ix, c, ids, orc.OracleMiekki.deserialize(want))
    finally:
        ix.close()


def qset_calls(ix, qs, n):
    """status of mk_qset_scores, mk_qset_run_compact and mk_qset_run_list on the set"""
    lib = ix._lib
    out = []
    d = C.c_void_p()
    assert lib.mk_dev_alloc(ix._h, max(n * max(ix.index_size, 1) * 4, n * 65 * 8, 16), C.byref(d)) == 0
    try:
        out.append(lib.mk_qset_scores(ix._h, qs, 0, n, d))
        out.append(lib.mk_qset_run_compact(ix._h, qs, 10, 10, 0.5 * THR, 64, d))
        hl = C.c_void_p()
        out.append(lib.mk_qset_run_list(ix._h, qs, 0xffffffff, 10, 0.5 * THR, C.byref(hl)))
        if out[-1] == 0:
            lib.mk_hitlist_free(hl)
        assert lib.mk_sync(ix._h) == 0
    finally:
        lib.mk_dev_free(ix._h, d)
    return out


def test_query_sets_across_a_select(hip, colls):
    from miekki_amd import lib as L
    from oracle import oracle as orc
    c = colls("C")
    ids = id_lists("C")["drop_each_third"]
    ix = c.build(hip)
    lib = ix._lib
    from_index, from_cols, uploaded, d_cols = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        low = np.array([0, 1, 5], np.uint32)                        # all below the new size: only the identity counter can tell
        L.check(lib.mk_qset_from_index(ix._h, low.ctypes.data, 3, C.byref(from_index)))
        assert qset_calls(ix, from_index, 3) == [0, 0, 0]
        L.check(lib.mk_dev_alloc(ix._h, (1 << c.h) * 3 * c.W, C.byref(d_cols)))
        L.check(lib.mk_index_export_genomes_device(ix._h, low.ctypes.data, 3, d_cols))
        L.check(lib.mk_qset_from_columns(ix._h, d_cols, 3, C.byref(from_cols)))
        seqs = [c.seqs[int(g)] for g in low]
        ptrs, lens = L.seq_arrays(seqs)
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, 3, C.byref(uploaded)))
        ix.select(ids)
        assert qset_calls(ix, from_index, 3) == [MK_ERR_STATE] * 3
        o2 = orc.OracleMiekki.deserialize(c.stream(ids))
        rows = o2.query_sequences(seqs)
        n = len(ids)
        for qs in (from_cols, uploaded):
            got = np.zeros((3, n), np.uint32)
            d = C.c_void_p()
            L.check(lib.mk_dev_alloc(ix._h, got.nbytes, C.byref(d)))
            try:
                L.check(lib.mk_qset_scores(ix._h, qs, 0, 3, d))
                L.check(lib.mk_sync(ix._h))
                L.check(lib.mk_dev_download(ix._h, got.ctypes.data, d, got.nbytes))
            finally:
                lib.mk_dev_free(ix._h, d)
            np.testing.assert_array_equal(got, rows)
            hl = C.c_void_p()
            L.check(lib.mk_qset_run_list(ix._h, qs, L.ALL_RESULTS, 10, 0.5 * THR, C.byref(hl)))
            same_hits(ix._hitlist(hl, 3), o2, rows, n)
        # a set made from the NEW index works, and one made before mk_index_import_begin does not
        fresh = C.c_void_p()
        L.check(lib.mk_qset_from_index(ix._h, low.ctypes.data, 3, C.byref(fresh)))
        assert qset_calls(ix, fresh, 3) == [0, 0, 0]
        L.check(lib.mk_index_import_begin(ix._h, n))
        assert qset_calls(ix, fresh, 3) == [MK_ERR_STATE] * 3
        lib.mk_qset_free(ix._h, fresh)
    finally:
        for qs in (from_index, from_cols, uploaded):
            if qs:
                lib.mk_qset_free(ix._h, qs)
        if d_cols:
            lib.mk_dev_free(ix._h, d_cols)
        ix.close()


def test_bad_lists_leave_the_index_as_it_was(hip, colls):
    c = colls("C")
    ix = c.build(hip)
    lib = ix._lib
    try:
        ix.file_names = [f"g{g}" for g in range(c.G)]
        want = c.stream(range(c.G))
        for ids in ([], [c.G], [3, 9, 3], [0, 1, c.G + 7]):
            a = np.array(ids, np.uint32)
            assert lib.mk_index_select(ix._h, a.ctypes.data, len(a)) == MK_ERR_ARG, ids
            with pytest.raises(hip.lib.MiekkiHipError):
                ix.select(ids)
        assert lib.mk_index_select(ix._h, None, 3) == MK_ERR_ARG
        assert ix.index_size == c.G and ix.file_names == [f"g{g}" for g in range(c.G)]
        stream_equals(ix, want)
    finally:
        ix.close()


def test_ids_follow_the_genome_id_base(hip, colls):
    c = colls("C")
    ix = hip.Miekki(*c.par, genome_id_base=1000)
    try:
        ix.insert_sequences(c.seqs)
        ids = id_lists("C")["random_subset"]
        a = np.array(ids[:5], np.uint32)
        assert ix._lib.mk_index_select(ix._h, a.ctypes.data, 5) == MK_ERR_ARG         # (local ids are not the context's)
        ix.select([1000 + g for g in ids])
        stream_equals(ix, c.stream(ids))
        hits, _ = ix.query([c.seqs[ids[0]]], 10, 10, 0.5 * THR)
        assert 1000 in {x.genome for x in hits[0]} and all(1000 <= x.genome < 1000 + len(ids) for x in hits[0])
    finally:
        ix.close()
