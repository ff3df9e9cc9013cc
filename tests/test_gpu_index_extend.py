"""mk_index_extend / Miekki.extend: the genomes of one index behind those of another, on the device.

The reference has no finished member for it (Miekki::merge_indexes, Miekki.cpp:901-910, forgets the sizes and the filter),
so the yardstick is the build itself: a collection is built ONCE in the oracle, cut at c, seqs[:c] and seqs[c:] are built on
the GPU as two indexes and joined, and serialize() must be the oracle's stream of the whole list byte for byte -- columns,
genome_size, Bloom filter, sketch_size.  The cuts are the places where extend_place_kernel changes path: destination
offsets 1 / 15 / 0 / 1 modulo 16, both sides of the 1 KiB piece and of the pitch, a 16-byte span that holds no aligned
word, a 15-byte span, a 1-byte span."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG, MK_ERR_UNSUPPORTED, MK_ERR_STATE = 0, -1, -2, -5
K, B, THR = 21, 32, 10


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


class Coll:
    """distinct genomes (every fourth shares its first half with the one before it, so that queries hit more than
    themselves), and the oracle's stream of the whole list: the yardstick of every cut"""

    def __init__(self, name, G, fp_bits, h, length):
        from oracle import oracle as orc
        self.name, self.G, self.fp_bits, self.h, self.W = name, G, fp_bits, h, fp_bits // 8
        self.par = (K, h, fp_bits, B, THR)
        self.seqs = []
        for g in range(G):
            s = synth.genome_bases(940_000 + 7 * G + g, 0, length + 3 * (g % 37))
            if g % 4 == 3:
                s = self.seqs[-1][:length // 2] + s[length // 2:]
            self.seqs.append(s)
        assert len(set(self.seqs)) == G
        self.extra = [synth.genome_bases(995_000 + g, 0, length) for g in range(2)]      # appended after a join
        self.o = orc.OracleMiekki(*self.par)
        self.o.insert_sequences(self.seqs)
        self.want = self.o.serialize()
        self.ss, self.gs = self.o.sketch_size, self.o.genome_size
        self._want_extra = None

    def want_extra(self):
        """the oracle's stream of the whole list plus the two extra genomes"""
        if self._want_extra is None:
            from oracle import oracle as orc
            o = orc.OracleMiekki(*self.par)
            o.insert_sequences(self.seqs + self.extra)
            self._want_extra = o.serialize()
        return self._want_extra


SHAPES = {"A": (1100, 8, 10, 2000),      # one byte per genome: crosses the 1 KiB piece and the 1 KiB pitch at 1,024 genomes
          "B": (600, 16, 10, 2000)}      # two bytes per genome: crosses them at 512
CUTS = {"A": (1, 15, 16, 17, 1023, 1024, 1025, 1084, 1085, 1099),
        "B": (1, 7, 8, 9, 511, 512, 513, 593, 599)}


@pytest.fixture(scope="module")
def colls():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Coll(name, *SHAPES[name])
        return made[name]
    return get


def build(hip, c, seqs, names=None, **kw):
    ix = hip.Miekki(*c.par, **kw)
    for i in range(0, len(seqs), 64):
        ix.insert_sequences(seqs[i:i + 64], names[i:i + 64] if names else None)
    return ix


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


def digest(ix):
    d = hashlib.blake2b()
    for piece in ix.serialize():
        d.update(piece)
    return d.digest()


def same_hits(got, o, rows, nres):
    """bit for bit: genome, matches, jaccard, intersection"""
    for q, row in enumerate(rows):
        assert [tuple(x) for x in got[q]] == o.filter_results(row, nres, 10, 0.5 * THR), q


@pytest.mark.parametrize("name,cut", [(n, c) for n in CUTS for c in CUTS[n]])
def test_join_is_the_joint_build(hip, colls, name, cut):
    c = colls(name)
    dst = build(hip, c, c.seqs[:cut], [f"g{g}" for g in range(cut)])
    src = build(hip, c, c.seqs[cut:], [f"g{g}" for g in range(cut, c.G)])
    try:
        dst.extend(src)
        assert dst.index_size == c.G and src.index_size == c.G - cut
        assert dst.file_names == [f"g{g}" for g in range(c.G)]
        np.testing.assert_array_equal(dst.sketch_size, c.ss)
        np.testing.assert_array_equal(dst.genome_size, c.gs)
        np.testing.assert_array_equal(src.sketch_size, c.ss[cut:])
        stream_equals(dst, c.want)
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("name,cut", [("A", 17), ("B", 513)])
def test_a_reserved_index_gives_the_same_stream(hip, colls, name, cut):
    """test_join_is_the_joint_build grows dst inside the call (at these cuts the matrix is laid out again); here it has the
    room beforehand"""
    c = colls(name)
    dst = hip.Miekki(*c.par)
    dst.reserve(c.G)
    for i in range(0, cut, 64):
        dst.insert_sequences(c.seqs[i:min(cut, i + 64)])
    src = build(hip, c, c.seqs[cut:])
    try:
        dst.extend(src)
        assert dst.file_names == [""] * c.G
        stream_equals(dst, c.want)
    finally:
        dst.close(); src.close()


def test_src_keeps_its_content_and_stays_usable(hip, colls):
    c = colls("B")
    cut = 9
    dst, src = build(hip, c, c.seqs[:cut]), build(hip, c, c.seqs[cut:])
    try:
        before = digest(src)
        dst.extend(src)
        assert digest(src) == before
        hits, _ = src.query([c.seqs[cut + 2]], 10, 10, 0.5 * THR)
        assert hits[0] and hits[0][0].genome == 2
        dst.file_names = []                                          # (not complete: the result has none)
        dst.extend(src)                                              # a second time: the same genomes once more, as another build would
        assert dst.index_size == 2 * c.G - cut and dst.file_names == []
        np.testing.assert_array_equal(dst.sketch_size, np.concatenate([c.ss, c.ss[cut:]]))
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("name,cuts", [("A", (15, 1039)), ("B", (8, 15))])
def test_three_parts_one_after_the_other(hip, colls, name, cuts):
    c = colls(name)
    a, b = cuts
    ix = build(hip, c, c.seqs[:a])
    try:
        for part in (c.seqs[a:b], c.seqs[b:]):
            other = build(hip, c, part)
            try:
                ix.extend(other)
            finally:
                other.close()
        stream_equals(ix, c.want)
    finally:
        ix.close()


@pytest.mark.parametrize("name,cut", [("A", 1025), ("B", 7)])
def test_an_append_after_a_join_is_still_a_joint_build(hip, colls, name, cut):
    """stale Bloom summaries or first-writer keys, a dirty tail behind the joined columns or stale sizes would show here"""
    c = colls(name)
    dst, src = build(hip, c, c.seqs[:cut]), build(hip, c, c.seqs[cut:])
    try:
        dst.extend(src)
        dst.insert_sequences(c.extra)
        assert dst.index_size == c.G + 2
        stream_equals(dst, c.want_extra())
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("name,cut,cold,packed", [("A", 1025, "dst", False), ("A", 1025, "dst", True), ("A", 17, "src", False),
                                                  ("A", 17, "both", False), ("B", 9, "both", False)])
def test_join_with_cold_rows(hip, colls, monkeypatch, name, cut, cold, packed):
    """rows beyond a 1 MiB budget live in page-locked host memory (1,024 rows at a pitch of 2 KiB: 512 stay in HBM) -- on
    dst only, on src only, on both, and on a dst whose cold rows were packed first: the same stream each time"""
    c = colls(name)

    def make(seqs, is_cold):
        if is_cold:
            monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")        # (read when the context is made)
        else:
            monkeypatch.delenv("MIEKKI_HBM_MATRIX_MIB", raising=False)
        return build(hip, c, seqs)
    dst = make(c.seqs[:cut], cold in ("dst", "both"))
    src = make(c.seqs[cut:], cold in ("src", "both"))
    try:
        if packed:
            dst.compress_index()
        dst.extend(src)
        stream_equals(dst, c.want)
    finally:
        dst.close(); src.close()


def test_queries_after_a_join(hip, colls):
    c = colls("A")
    cut = 1023
    dst, src = build(hip, c, c.seqs[:cut]), build(hip, c, c.seqs[cut:])
    try:
        dst.extend(src)
        qs = [c.seqs[g][100:1500] for g in (0, 3, cut - 1, cut, cut + 1, c.G - 1)] + [c.seqs[cut - 2], synth.genome_bases(998_000, 0, 1500)]
        rows = c.o.query_sequences(qs)
        assert rows[:-1].max(axis=1).min() >= 10                     # every related query has something to report
        np.testing.assert_array_equal(dst.query_sequences(qs), rows)
        hits, act = dst.query(qs, 10, 10, 0.5 * THR)
        same_hits(hits, c.o, rows, 10)
        assert [int(a) for a in act] == [c.o.query_sequence(s)[1] for s in qs]
        assert any(x.genome >= cut for h in hits for x in h) and any(x.genome < cut for h in hits for x in h)
    finally:
        dst.close(); src.close()


def test_a_set_from_the_index_runs_across_a_join(hip, colls):
    """the ids of dst's genomes mean what they meant: MK_OK, not MK_ERR_STATE, and the list holds the joined genomes"""
    from miekki_amd import lib as L
    from oracle import oracle as orc
    c = colls("A")
    # genomes 2 and 6 of the collection first, then the genomes that share half of them (3 and 7) among others: the lists of
    # ids 0 and 1 grow by the join
    seqs = [c.seqs[2], c.seqs[6], c.seqs[3], c.seqs[7]] + c.seqs[8:40]
    cut = 2
    o = orc.OracleMiekki(*c.par)
    o.insert_sequences(seqs)
    dst, src = build(hip, c, seqs[:cut]), build(hip, c, seqs[cut:])
    lib = dst._lib
    qs = C.c_void_p()
    try:
        ids = np.array([0, 1], np.uint32)
        L.check(lib.mk_qset_from_index(dst._h, ids.ctypes.data, 2, C.byref(qs)))
        hl = C.c_void_p()
        assert lib.mk_qset_run_list(dst._h, qs, L.ALL_RESULTS, 10, 0.5 * THR, C.byref(hl)) == MK_OK
        first = dst._hitlist(hl, 2)
        assert all(row and all(x.genome < cut for x in row) for row in first)
        assert lib.mk_index_extend(dst._h, src._h) == MK_OK
        hl = C.c_void_p()
        assert lib.mk_qset_run_list(dst._h, qs, L.ALL_RESULTS, 10, 0.5 * THR, C.byref(hl)) == MK_OK
        after = dst._hitlist(hl, 2)
        rows = np.stack([o.query_sequence(seqs[g])[0] for g in (0, 1)])
        same_hits(after, o, rows, len(seqs))
        assert 2 in {x.genome for x in after[0]} and 3 in {x.genome for x in after[1]}
    finally:
        if qs:
            lib.mk_qset_free(dst._h, qs)
        dst.close(); src.close()


def test_refusals_leave_the_index_as_it_was(hip, colls):
    c = colls("B")
    dst = build(hip, c, c.seqs[:40], [f"g{g}" for g in range(40)])
    lib = dst._lib
    others = []
    try:
        before = digest(dst)
        for par, word in (((K - 1, c.h, c.fp_bits, B, THR), b" k "), ((K, c.h - 1, c.fp_bits, B, THR), b" h "),
                          ((K, c.h, 8, B, THR), b" fp_bits "), ((K, c.h, c.fp_bits, B + 1, THR), b" bloom_log2 ")):
            o = hip.Miekki(*par)
            others.append(o)
            o.insert_sequences(c.seqs[40:43])
            assert lib.mk_index_extend(dst._h, o._h) == MK_ERR_ARG, par
            assert word in lib.mk_last_error(), (par, lib.mk_last_error())
            with pytest.raises(hip.lib.MiekkiHipError):
                dst.extend(o)
        assert lib.mk_index_extend(dst._h, dst._h) == MK_ERR_ARG
        assert lib.mk_index_extend(dst._h, None) == MK_ERR_ARG
        assert lib.mk_index_extend(None, dst._h) == MK_ERR_ARG
        with pytest.raises(hip.lib.MiekkiHipError):
            dst.extend(dst)
        empty = hip.Miekki(*c.par)
        others.append(empty)
        assert lib.mk_index_extend(dst._h, empty._h) == MK_OK       # an empty src: nothing changes
        dst.extend(empty)
        assert dst.index_size == 40 and dst.file_names == [f"g{g}" for g in range(40)]
        assert digest(dst) == before
    finally:
        dst.close()
        for o in others:
            o.close()


def test_an_empty_dst_becomes_src_under_its_own_header(hip, colls):
    c = colls("B")
    src = build(hip, c, c.seqs)
    dst = hip.Miekki(K, c.h, c.fp_bits, B, THR + 67, genome_id_base=500)
    try:
        dst.extend(src)
        want = c.want.copy()
        want[34:38] = np.frombuffer(np.uint32(THR + 67).tobytes(), np.uint8)      # the header's threshold: dst's own
        stream_equals(dst, want)
        hits, _ = dst.query([c.seqs[5]], 10, 10, 0.5 * THR)
        assert hits[0][0].genome == 505                              # ... and its own genome_id_base
    finally:
        dst.close(); src.close()


def test_indexes_on_two_devices_are_refused(hip, colls):
    lib = hip.lib.load_library()
    if lib.mk_device_count() < 2:
        pytest.skip("needs two GPUs")
    c = colls("B")
    dst = build(hip, c, c.seqs[:5])
    src = build(hip, c, c.seqs[5:9], device=1)
    try:
        before = digest(dst)
        assert lib.mk_index_extend(dst._h, src._h) == MK_ERR_UNSUPPORTED
        assert digest(dst) == before
    finally:
        dst.close(); src.close()
