"""mk_cover_gather / mk_query_cover_gather and Miekki.gather: the greedy set cover over a cover table must be, pick for pick and
field for field, what tests/gather_ref.py's numpy loop makes of the ORACLE's gated sketches and stored columns: P = 512,
G = 1,101 at one byte (more than one workgroup of the pick step, no multiple of 1,024) and 603 at two, hundreds of rounds of
which most are decided by the tie-break."""
import ctypes as C

import numpy as np
import pytest

import cover_ref as cr
import depth_ref as dr
import gather_ref as gr
import synth
import winners_ref as wr

pytestmark = pytest.mark.gpu
MK_OK, MK_ERR_ARG = 0, -1
WIDTHS = [8, 16]
SWITCHES = ("MIEKKI_GATHER_ROUNDS", "MIEKKI_GATHER_RECOUNT")


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def check(st):
    from miekki_amd import lib as L
    L.check(st)


@pytest.fixture(scope="module")
def samples():
    return wr.samples()


@pytest.fixture(scope="module")
def runs(samples):
    return gr.runs(samples)


@pytest.fixture(scope="module")
def mults(samples):
    """int64 [P, 2^bits] per width: in how many reads of the sample each cell turns up (depth_ref), made once"""
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = dr.mult(samples(bits).o, samples(bits).s.queries)
        return made[bits]
    return get


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


class DevBuf:
    def __init__(self, ix, nbytes):
        self.ix, self.p, self.nbytes = ix, C.c_void_p(), nbytes
        check(ix._lib.mk_dev_alloc(ix._h, max(nbytes, 32), C.byref(self.p)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def close(self):
        if self.p:
            self.ix._lib.mk_dev_free(self.ix._h, self.p)
        self.p = None

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.nbytes
        check(self.ix._lib.mk_dev_upload(self.ix._h, self.p, arr.ctypes.data, arr.nbytes))
        return self

    def download(self):
        out = np.empty(self.nbytes, np.uint8)
        check(self.ix._lib.mk_dev_download(self.ix._h, out.ctypes.data, self.p, self.nbytes))
        return out


def marked(ix, *sets, depth=False):
    """(cover table, depth table or None) of the index's own sizes, reset, with the sets of sequences marked into them"""
    lib = ix._lib
    seen = DevBuf(ix, lib.mk_cover_bytes(ix._h))
    mult = DevBuf(ix, lib.mk_depth_bytes(ix._h)) if depth else None
    check(lib.mk_cover_reset(ix._h, seen.p))
    if mult:
        check(lib.mk_depth_reset(ix._h, mult.p))
    for seqs in sets:
        qs, n = C.c_void_p(), len(seqs)
        ptrs, lens = (C.c_char_p * n)(*seqs), (C.c_uint64 * n)(*[len(s) for s in seqs])
        check(lib.mk_qset_upload(ix._h, ptrs, lens, n, C.byref(qs)))
        try:
            check(lib.mk_qset_run_cover(ix._h, qs, seen.p))
            if mult:
                check(lib.mk_qset_run_depth(ix._h, qs, mult.p))
        finally:
            lib.mk_qset_free(ix._h, qs)
    return seen, mult


@pytest.fixture(scope="module")
def indexes(hip, samples, mults):
    """per width: the sample, its index, and the yardstick's own tables uploaded: (w, ix, seen, mult)"""
    made = {}

    def get(bits):
        if bits not in made:
            w = samples(bits)
            ix = w.s.a.build(hip)
            seen = DevBuf(ix, w.nbytes).upload(w.words)
            mult = DevBuf(ix, w.nbytes * 8).upload(dr.table(mults(bits)))
            made[bits] = (w, ix, seen, mult)
        return made[bits]
    yield get
    for w, ix, seen, mult in made.values():
        seen.close()
        mult.close()
        ix.close()


def gather(ix, seen, mult=None, min_new=1, max_picks=0):
    """mk_cover_gather: (picks, cells, explained); the room behind the picks made must stay as it was"""
    room = min(max_picks, ix.index_size) if max_picks else ix.index_size
    picks = np.zeros(room + 1, gr.PICK)
    picks[:] = (0xdead, 0xdead, 0xdead, 0xdead, 0xdead)
    n, cells, explained = C.c_uint32(0xdead), C.c_uint64(0xdead), C.c_uint64(0xdead)
    check(ix._lib.mk_cover_gather(ix._h, seen.p, mult.p if mult else None, min_new, max_picks, picks.ctypes.data, C.byref(n),
                                  C.byref(cells), C.byref(explained)))
    assert n.value <= room and (picks["genome"][n.value:] == 0xdead).all()
    return picks[:n.value].copy(), int(cells.value), int(explained.value)


def same(got, want):
    for f in gr.PICK.names:
        np.testing.assert_array_equal(got[0][f], want[0][f], err_msg=f)
    assert len(got[0]) == len(want[0]) and got[1:] == want[1:]


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("min_new", [1, 10, 40])
@pytest.mark.parametrize("bits", WIDTHS)
def test_like_the_yardstick(indexes, runs, mults, bits, min_new, depth):
    w, ix, seen, mult = indexes(bits)
    ix.reset_stats()
    got = gather(ix, seen, mult if depth else None, min_new)
    assert ix.stats()["filter_ms"] > 0                                     # the gather's kernels are carried by filter_ms
    want = runs(bits).picks(min_new, table=dr.table(mults(bits)) if depth else None)
    assert len(want[0]) > 100
    same(got, want)
    if min_new == 1:
        assert got[2] == w.claimed                                         # -W's claimed


@pytest.mark.parametrize("max_picks", [1, 7])
@pytest.mark.parametrize("bits", WIDTHS)
def test_a_cap(indexes, runs, mults, bits, max_picks):
    w, ix, seen, mult = indexes(bits)
    got = gather(ix, seen, mult, 1, max_picks)
    assert len(got[0]) == max_picks
    same(got, runs(bits).picks(1, max_picks, dr.table(mults(bits))))
    same(gather(ix, seen, None, 40, max_picks), runs(bits).picks(40, max_picks))
    same(gather(ix, seen, None, 1, 0xffffffff), runs(bits).picks())        # a cap beyond G is no cap


@pytest.mark.parametrize("bits", WIDTHS)
def test_from_sequences_in_one_call(indexes, runs, mults, bits):
    """mk_query_cover_gather through Miekki.gather: the marks, the count and the rounds; with and without a depth table"""
    w, ix, _, _ = indexes(bits)
    run, tab = runs(bits), dr.table(mults(bits))
    got = ix.gather(w.s.queries)
    assert got[0].dtype == gr.PICK
    same(got, run.picks(10))
    same(ix.gather(w.s.queries, min_new=40, depth=True), run.picks(40, table=tab))
    same(ix.gather(w.s.queries, 1, 7, True), run.picks(1, 7, tab))
    # outputs are written, not accumulated; cells and explained may be NULL
    q = w.s.queries[:40]
    ptrs, lens = (C.c_char_p * len(q))(*q), (C.c_uint64 * len(q))(*[len(s) for s in q])
    picks = np.zeros(w.G, gr.PICK)
    n = C.c_uint32(99)
    check(ix._lib.mk_query_cover_gather(ix._h, ptrs, lens, len(q), 1, 1, 0, picks.ctypes.data, C.byref(n), None, None))
    seen_q = cr.seen(w.o, q)
    want = gr.gather(w.o, seen_q, w.fps, table=dr.table(dr.mult(w.o, q)))
    assert 0 < n.value == len(want[0]) < len(run.rounds)
    np.testing.assert_array_equal(picks[:n.value], want[0])


@pytest.mark.parametrize("bits", WIDTHS)
def test_reads_split_into_sets_and_given_twice(indexes, runs, mults, bits):
    """the bit table is an OR: the picks stay; the byte table adds up to its cap: depth_sum doubles, as the yardstick says"""
    w, ix, _, _ = indexes(bits)
    q, run, m = w.s.queries, runs(bits), mults(bits)
    seen, mult = marked(ix, q[:300], q[300:], depth=True)
    try:
        same(gather(ix, seen, mult), run.picks(table=dr.table(m)))
    finally:
        seen.close(), mult.close()
    seen, mult = marked(ix, q, q[:300], q[300:], depth=True)
    try:
        assert 2 * m.max() < dr.DEPTH_MAX
        twice = run.picks(10, table=dr.table(2 * m))
        np.testing.assert_array_equal(twice[0]["depth_sum"], 2 * run.picks(10, table=dr.table(m))[0]["depth_sum"])
        same(gather(ix, seen, mult, 10), twice)
    finally:
        seen.close(), mult.close()
    times = 5 if bits == 8 else 10                                         # (the largest mult is 65 and 28)
    seen, mult = marked(ix, *[q] * times, depth=True)                      # some cells at the cap, others not
    try:
        capped = dr.table(times * m)
        assert (capped == 255).any() and ((capped > 0) & (capped < 255)).any()
        same(gather(ix, seen, mult, 40), run.picks(40, table=capped))
    finally:
        seen.close(), mult.close()


@pytest.mark.parametrize("switch,value", [("MIEKKI_GATHER_ROUNDS", "1"), ("MIEKKI_GATHER_ROUNDS", "3"), ("MIEKKI_GATHER_ROUNDS", "1000"),
                                          ("MIEKKI_GATHER_RECOUNT", "1")])
@pytest.mark.parametrize("bits", WIDTHS)
def test_rounds_per_wait_and_the_recount_route_give_the_same_picks(indexes, runs, mults, monkeypatch, bits, switch, value):
    w, ix, seen, mult = indexes(bits)
    tab = dr.table(mults(bits))
    default = gather(ix, seen, mult, 10)
    monkeypatch.setenv(switch, value)
    same(gather(ix, seen, mult, 10), default)
    same(default, runs(bits).picks(10, table=tab))
    same(gather(ix, seen, mult, 1, 7), runs(bits).picks(1, 7, tab))        # a cap in the middle of a batch of rounds
    if switch == "MIEKKI_GATHER_RECOUNT":
        monkeypatch.setenv("MIEKKI_GATHER_ROUNDS", "5")                    # the count pass goes on behind the stop
        same(gather(ix, seen, mult, 40), runs(bits).picks(40, table=tab))


@pytest.mark.parametrize("bits", WIDTHS)
def test_the_callers_tables_are_not_modified(indexes, runs, bits):
    w, ix, seen, mult = indexes(bits)
    before = seen.download(), mult.download()
    first = gather(ix, seen, mult)
    second = gather(ix, seen, mult)
    np.testing.assert_array_equal(seen.download(), before[0])
    np.testing.assert_array_equal(mult.download(), before[1])
    np.testing.assert_array_equal(before[0].view(np.uint32), w.words)
    same(second, first)
    assert len(first[0]) == len(runs(bits).rounds)


@pytest.mark.parametrize("bits", WIDTHS)
def test_uploaded_tables_all_ones_and_all_zero(indexes, bits):
    """every bit set: every stored fingerprint is live, the bit of `empty` counts for nothing, and the rows' zero padding
    equals v = 0: with the cells (p, 0) alone set -- no stored fingerprint of the samples is 0 -- the padding columns are the
    only "holders" there are, and nothing may be picked.  No bit set: no pick."""
    w, ix, _, mult = indexes(bits)
    ones = np.ones((w.P, 1 << bits), bool)
    want = gr.gather(w.o, ones, w.fps, max_picks=40)
    assert want[0]["fresh"][0] == np.asarray(w.o.sketch_size).max() and want[1] == w.P << bits
    zeros_only = np.zeros((w.P, 1 << bits), bool)
    zeros_only[:, 0] = True
    want_0 = gr.gather(w.o, zeros_only, w.fps, max_picks=60)
    assert not (w.fps == 0).any() and len(want_0[0]) == 0 and want_0[1:] == (w.P, 0)
    with DevBuf(ix, w.nbytes) as tab:
        tab.upload(np.full(w.nbytes // 4, 0xffffffff, np.uint32))
        same(gather(ix, tab, None, 1, 40), want)
        tab.upload(cr.pack(zeros_only))
        same(gather(ix, tab, None, 1, 60), want_0)
        tab.upload(np.zeros(w.nbytes // 4, np.uint32))
        got = gather(ix, tab, mult)
        assert len(got[0]) == 0 and got[1:] == (0, 0)
        only_empty = np.zeros((w.P, 1 << bits), bool)
        only_empty[:, cr.empty_of(w.o)] = True
        tab.upload(cr.pack(only_empty))
        got = gather(ix, tab, mult)
        assert len(got[0]) == 0 and got[1:] == (w.P, 0)


@pytest.mark.parametrize("bits", WIDTHS)
def test_five_thousand_genomes_span_many_workgroups(hip, bits):
    """5,003 device-synthetic genomes in families of 16: twenty workgroups of the pick step, rows of five (ten) tiles and a
    ragged last one, two runs of tiles per list entry at two bytes.  No oracle at this size: the yardstick's loop over the
    index's own exported columns and an uploaded seeded random table, `empty`'s bits set among the others."""
    G, P, rounds = 5003, 512, 24
    ix = hip.Miekki(15, 9, bits, 32, 20)
    try:
        ix.insert_synthetic_strains(0, G, 3000, 16, 20000)
        cols = np.empty(P * G * bits // 8, np.uint8)
        check(ix._lib.mk_index_export_columns(ix._h, 0, P, cols.ctypes.data))
        fps = (cols if bits == 8 else cols.view(">u2")).reshape(P, G).astype(np.int64)
        empty = (1 << bits) - 1
        ss = np.asarray(ix.sketch_size)
        np.testing.assert_array_equal((fps != empty).sum(0), ss)
        rng = np.random.default_rng(5003 + bits)
        table = rng.random((P, 1 << bits)) < 0.4
        table[::3, empty] = True
        table[:, 0] = True                                                 # the padding's value: live in every row
        print("stored fingerprints equal to 0:", int((fps == 0).sum()))
        rem0 = (table[np.arange(P)[:, None], fps] & (fps != empty)).sum(0)
        mult_tab = rng.integers(1, 256, P << bits, dtype=np.uint8)
        nbytes = (P << bits) >> 3
        with DevBuf(ix, nbytes) as seen, DevBuf(ix, nbytes * 8) as mult:
            seen.upload(cr.pack(table))
            mult.upload(mult_tab)
            for min_new, cap in ((1, rounds), (int(rem0.max()) - 2, 0)):
                want_rounds = gr.loop(P, G, bits, table, fps, min_new, cap)
                want = gr.picks_of(want_rounds, rem0, ss, mult_tab)
                assert 0 < len(want) and (cap == 0 or len(want) == rounds)
                got = gather(ix, seen, mult, min_new, cap)
                same(got, (want, int(table.sum()), int(want["fresh"].sum())))
    finally:
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_imported_columns_full_of_zero_fingerprints(hip, monkeypatch, bits):
    """the padding trap in the strike step: columns imported as they are (mk_index_import_columns), fingerprints drawn from
    0..5 and `empty`, so that a pick strikes cells (p, 0) in a sixth of its rows, each of which equals the zero padding of
    columns [G, pitch) -- 947 (421) of them.  Counting those down would write behind rem[G) and, at one byte, wrap the count
    of nobody; the yardstick's loop over the same columns must be met pick for pick."""
    P, G = 512, 1101 if bits == 8 else 603
    empty = (1 << bits) - 1
    rng = np.random.default_rng(1101 + bits)
    fps = rng.integers(0, 7, (P, G)).astype(np.int64)
    fps[fps == 6] = empty
    fps[:, G // 2] = 0                                                     # one genome of zeros alone: the first pick
    cols = fps.astype(np.uint8) if bits == 8 else fps.astype(">u2").view(np.uint8)
    ss = (fps != empty).sum(0).astype(np.uint32)
    gs = np.full(G, 100_000, np.uint64)
    ix = hip.Miekki(15, 9, bits, 32, 20)
    try:
        lib = ix._lib
        cols = np.ascontiguousarray(cols).reshape(-1)
        check(lib.mk_index_import_begin(ix._h, G))
        check(lib.mk_index_import_columns(ix._h, 0, P, cols.ctypes.data))
        check(lib.mk_index_import_sizes(ix._h, gs.ctypes.data, ss.ctypes.data))
        assert lib.mk_index_size(ix._h) == G
        table = np.zeros((P, 1 << bits), bool)
        table[:, :6] = rng.random((P, 6)) < 0.8
        table[:, 0] = True
        table[:, empty] = True
        rem0 = (table[np.arange(P)[:, None], fps] & (fps != empty)).sum(0)
        rounds = gr.loop(P, G, bits, table, fps, max_picks=30)
        assert rounds[0][0] == G // 2 and rounds[0][1] == P and ((rounds[0][2] & empty) == 0).all()   # every (p, 0) struck at once
        want = gr.picks_of(rounds, rem0, ss)
        nbytes = (P << bits) >> 3
        with DevBuf(ix, nbytes) as seen:
            seen.upload(cr.pack(table))
            room = np.zeros(31, gr.PICK)
            n, cells, explained = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
            for recount in (False, True):
                if recount:
                    monkeypatch.setenv("MIEKKI_GATHER_RECOUNT", "1")
                check(lib.mk_cover_gather(ix._h, seen.p, None, 1, 30, room.ctypes.data, C.byref(n), C.byref(cells), C.byref(explained)))
                same((room[:n.value], int(cells.value), int(explained.value)), (want, int(table.sum()), int(want["fresh"].sum())))
    finally:
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_cold_rows_raw_and_packed(hip, samples, runs, mults, monkeypatch, bits):
    """1 MiB of a 2 MiB matrix in HBM (a reservation doubles the rows' pitch), the other rows in host memory: read where they
    lie; then packed (compress_index), which the call unpacks first"""
    w, run, tab = samples(bits), runs(bits), dr.table(mults(bits))
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    ix = hip.Miekki(*w.s.c.par)
    try:
        ix.reserve(4096 * 8 // bits)
        for i in range(0, w.G, 64):
            ix.insert_sequences(w.s.c.seqs[i:i + 64])
        same(ix.gather(w.s.queries, 10, depth=True), run.picks(10, table=tab))
        raw, packed = ix.compress_index()
        assert raw >= 1 << 20                                              # (there are cold rows)
        with DevBuf(ix, w.nbytes) as seen:
            seen.upload(w.words)
            same(gather(ix, seen, None, 10), run.picks(10))                # (unpacks)
            ix.compress_index()
            monkeypatch.setenv("MIEKKI_GATHER_RECOUNT", "1")
            same(gather(ix, seen, None, 40), run.picks(40))
    finally:
        ix.close()


def test_genome_is_the_reported_id(hip, samples, runs, mults):
    """genome_id_base 1000: the rounds go by local genome, the picks name the ids the context reports"""
    w, run = samples(8), runs(8)
    ix = w.s.a.build(hip, genome_id_base=1000)
    try:
        want = run.picks(10, table=dr.table(mults(8)), base=1000)
        assert want[0]["genome"].min() >= 1000
        same(ix.gather(w.s.queries, 10, depth=True), want)
        with DevBuf(ix, w.nbytes) as seen:
            seen.upload(w.words)
            same(gather(ix, seen, None, 10), run.picks(10, base=1000))
    finally:
        ix.close()


def test_refusals_leave_the_outputs_alone(indexes):
    w, ix, seen, mult = indexes(8)
    lib, G = ix._lib, w.G
    picks = np.zeros(G, gr.PICK)
    picks[:] = (7, 7, 7, 7, 7)
    n, cells, explained = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)
    out = (C.byref(n), C.byref(cells), C.byref(explained))
    q = w.s.queries[:2]
    ptrs, lens = (C.c_char_p * 2)(*q), (C.c_uint64 * 2)(*[len(s) for s in q])
    assert lib.mk_cover_gather(None, seen.p, mult.p, 1, 0, picks.ctypes.data, *out) == MK_ERR_ARG
    assert lib.mk_cover_gather(ix._h, None, mult.p, 1, 0, picks.ctypes.data, *out) == MK_ERR_ARG
    assert lib.mk_cover_gather(ix._h, seen.p, mult.p, 1, 0, None, *out) == MK_ERR_ARG
    assert lib.mk_cover_gather(ix._h, seen.p, mult.p, 1, 0, picks.ctypes.data, None, out[1], out[2]) == MK_ERR_ARG
    assert lib.mk_cover_gather(ix._h, seen.p, mult.p, 0, 0, picks.ctypes.data, *out) == MK_ERR_ARG
    assert b"min_new" in lib.mk_last_error()
    assert lib.mk_cover_gather(ix._h, seen.p, None, 0, 5, picks.ctypes.data, *out) == MK_ERR_ARG
    assert lib.mk_query_cover_gather(ix._h, None, None, 3, 0, 1, 0, picks.ctypes.data, *out) == MK_ERR_ARG
    assert lib.mk_query_cover_gather(ix._h, ptrs, lens, 2, 1, 0, 0, picks.ctypes.data, *out) == MK_ERR_ARG
    assert lib.mk_query_cover_gather(ix._h, ptrs, lens, 2, 1, 1, 0, None, *out) == MK_ERR_ARG
    assert lib.mk_query_cover_gather(ix._h, ptrs, lens, 2, 1, 1, 0, picks.ctypes.data, None, out[1], out[2]) == MK_ERR_ARG
    check(lib.mk_sync(ix._h))
    assert (n.value, cells.value, explained.value) == (7, 7, 7)
    assert all((picks[f] == 7).all() for f in gr.PICK.names)
    np.testing.assert_array_equal(seen.download().view(np.uint32), w.words)


def test_empty_index(hip):
    ix = hip.Miekki(15, 9, 8, 32, 20)
    try:
        reads = [synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)]
        picks, cells, explained = ix.gather(reads, depth=True)
        assert picks.shape == (0,) and picks.dtype == gr.PICK and cells == explained == 0
        lib = ix._lib
        n, c, e = C.c_uint32(99), C.c_uint64(99), C.c_uint64(99)
        table = np.arange(4096, dtype=np.uint32)
        with DevBuf(ix, 16384) as tab:
            tab.upload(table)
            assert lib.mk_cover_gather(ix._h, tab.p, None, 1, 0, None, C.byref(n), C.byref(c), C.byref(e)) == MK_OK
            assert (n.value, e.value) == (0, 0) and c.value == int(np.unpackbits(table.view(np.uint8)).sum())
            n = C.c_uint32(99)
            assert lib.mk_cover_gather(ix._h, tab.p, None, 3, 2, None, C.byref(n), None, None) == MK_OK and n.value == 0
            assert lib.mk_cover_gather(ix._h, tab.p, None, 0, 0, None, C.byref(n), None, None) == MK_ERR_ARG
    finally:
        ix.close()
