"""The dense scans' counters AT their limits, all n x G scores compared with exact integer numpy.

scan_dense_lut_kernel (scan_kernel.hpp) counts the matches of eight queries per mask word in 14 bit planes: sixteen rows go
in as eight pairs through carry-save adders (ones -> twos -> fours -> eights -> one carry of weight 16), planes 4-7 are
rippled in registers, a carry out of plane 7 is OR-ed into `pend` -- right only while a counter passes a multiple of 256 at
most once between two flushes --, `pend` is rippled through six planes in LDS every 256 rows and once after the last row
(flush_pending), the planes become numbers per query bit j by (pl >> j) & 0x01010101, and chunks of at most 16,368 rows
(dense_chunk_rows, mk_internal.hpp) are added to the score rows with atomics.  Two or four waves share the rows through LDS
(GS), one or two octets of queries run per wave (NO; launch_scan_dense, scan.hip), with clamped table pointers and idle
waves where the counts do not divide; at two bytes a match is both & (both >> 8) & 0x00ff00ff.  scan_dense_kernel takes
over where a window of rows is no multiple of 16, with a spill of its byte counters every 248 rows.

The inputs (dense_limits.py, proven by test_dense_limit_inputs.py) put steered columns at 0, 1, 15, 16, 17, 255, 256, 257,
511, 512, 4095, 4096, 4097, 8191, 8192, 16367 and 16368 matches within a chunk -- in its first rows, its last rows and
scattered --, at every row position of a block, on both sides of every flush and of the chunk edge.  The matrix goes in by
mk_index_import_columns, the queries by mk_qset_from_columns: no genome, no sketch and no oracle is involved.

There is no tolerance in this module: mk_qset_scores and mk_qset_active are compared with dense_limits.count by
np.testing.assert_array_equal, every entry.

Wall time of the module on an MI355X: about 5 s (32 tests; the slowest, 72 queries at one byte, half a second), most of it
numpy's side (building the inputs and counting them)."""
import numpy as np
import pytest

import dense_limits as dl
from test_gpu_from_index import DevBuf, QSet, hip_check

pytestmark = pytest.mark.gpu
WIDTHS = [8, 16]


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def new_context(hip, h, bits):
    return hip.Miekki(15, h, bits, 32, 20)                       # (k, the filter and the threshold play no part: nothing is sketched)


def load(ix, M, meta):
    """M as the index: columns as they are, sketch_size = the non-empty rows of a column, any genome_size"""
    if getattr(ix, "_loaded", None) is M:
        return
    P, G = M.shape
    cols = dl.to_dump(M, meta.bits)
    ss = (M != meta.empty).sum(0).astype(np.uint32)
    gs = np.full(G, 100_000, np.uint64)
    lib = ix._lib
    hip_check(lib.mk_index_import_begin(ix._h, G))
    hip_check(lib.mk_index_import_columns(ix._h, 0, P, cols.ctypes.data))
    hip_check(lib.mk_index_import_sizes(ix._h, gs.ctypes.data, ss.ctypes.data))
    assert lib.mk_index_size(ix._h) == G
    ix._loaded = M


@pytest.fixture(scope="module")
def contexts(hip):
    """one context per (h, bits); a case imports its matrix into it"""
    made = {}

    def get(h, bits):
        if (h, bits) not in made:
            made[h, bits] = new_context(hip, h, bits)
        return made[h, bits]
    yield get
    for ix in made.values():
        ix.close()


@pytest.fixture(scope="module")
def cases():
    """(Q, M, meta, scores, active) of a builder's case: built and counted once"""
    made = {}

    def get(name, *args):
        if (name, args) not in made:
            Q, M, meta = getattr(dl, name)(*args)
            scores, active, _ = dl.count(Q, M, meta.empty)
            scores.setflags(write=False)
            made[name, args] = (Q, M, meta, scores, active)
        return made[name, args]
    return get


class Columns:
    """Q on the device as a set of whole-genome queries"""

    def __init__(self, ix, Q, meta):
        self.ix, self.n = ix, Q.shape[1]
        self.dump = dl.to_dump(Q, meta.bits)

    def __enter__(self):
        self.buf = DevBuf(self.ix, self.dump.nbytes)
        self.buf.upload(self.dump)
        self.qs = QSet(self.ix, d_cols=self.buf.p, n=self.n)
        return self.qs

    def __exit__(self, *a):
        self.qs.__exit__()
        self.buf.__exit__()


def same(got, want, meta, what):
    """equality of every entry; the message names the steered columns among the first that differ"""
    got = np.asarray(got).astype(np.int64)
    if not np.array_equal(got, want):
        tags = {(s.q, s.col): s.tag for s in meta.steer}
        bad = np.argwhere(got != want)
        lines = [f"{what}: {len(bad)} of {want.size} scores differ; (query, column): device / yardstick"]
        steered = [b for b in bad if (int(b[0]), int(b[1])) in tags]
        for q, g in (steered + list(bad))[:12]:
            lines.append(f"  ({q}, {g}): {got[q, g]} / {want[q, g]}  {tags.get((int(q), int(g)), '')}")
        print("\n".join(lines))
    np.testing.assert_array_equal(got, want, err_msg=str(what))


def run_case(ix, case, what):
    Q, M, meta, scores, active = case
    load(ix, M, meta)
    with Columns(ix, Q, meta) as qs:
        got = qs.scores()
        same(got, scores, meta, what)
        np.testing.assert_array_equal(qs.active().astype(np.int64), active, err_msg=str(what))
    return got


def schedule(n):
    """(octets, NO, GS) of n queries, as launch_scan_dense and dense_share (mk_internal.hpp) have it: groups of four queries
    (the last padded), two groups to an octet, NO = 2 octets per wave when there are two, sets of NO octets, and GS = 4
    waves sharing a tile's rows from three sets on, 2 at two sets, else 1"""
    groups = -(-n // 4)
    octets = -(-groups // 2)
    no = 2 if octets >= 2 else 1
    sets = -(-octets // no)
    return octets, no, 4 if sets >= 3 else 2 if sets == 2 else 1


def test_the_schedules_the_cases_are_chosen_for():
    assert [schedule(n) for n in (8, 16, 24, 72)] == [(1, 1, 1), (2, 2, 1), (3, 2, 2), (9, 2, 4)]
    # 24: two sets, the second's second octet is the clamped one; 72: five sets in two sharing groups of four waves, three idle
    assert -(-3 // 2) == 2 and 2 * 2 - 3 == 1 and -(-9 // 2) == 5 and 2 * 4 - 5 == 3
    assert [schedule(n) for n in (1, 5, 9, 17, 33, 65)] == [(1, 1, 1), (1, 1, 1), (2, 2, 1), (3, 2, 2), (5, 2, 4), (9, 2, 4)]


# ---- a. the counters

@pytest.mark.parametrize("n", [8, 16, 24, 72])
@pytest.mark.parametrize("bits", WIDTHS)
def test_a_counters_on_every_schedule(contexts, cases, bits, n):
    run_case(contexts(14, bits), cases("planes", 14, bits, n), ("planes", 14, bits, n))


@pytest.mark.parametrize("bits", WIDTHS)
def test_a_three_chunks(contexts, cases, bits):
    """32,768 rows: chunks of 16,368 + 16,368 + 32; a column equal in every row sums to 32,768 across them"""
    got = run_case(contexts(15, bits), cases("planes", 15, bits, 16), ("planes", 15, bits, 16))
    assert int(got.max()) == 32768


@pytest.mark.parametrize("n", [1, 5, 9, 17, 33, 65])
def test_a_padded_groups(contexts, cases, n):
    """n no multiple of four: slots 0xffffffff in dense_q (queries that are `empty` in every row)"""
    run_case(contexts(14, 8), cases("planes", 14, 8, n), ("planes", 14, 8, n))


# ---- b. edges

@pytest.mark.parametrize("bits", WIDTHS)
def test_b_edges(contexts, cases, bits):
    run_case(contexts(14, bits), cases("edges", 14, bits), ("edges", bits))


@pytest.mark.parametrize("h", [3, 4, 8])
@pytest.mark.parametrize("bits", WIDTHS)
def test_b_small(contexts, cases, bits, h):
    """8 rows: the compare kernel; 16: one block of the table kernel; 256: the in-loop flush and the final one coincide"""
    run_case(contexts(h, bits), cases("small", h, bits), ("small", h, bits))


# ---- c. sub-ranges of the set

@pytest.mark.parametrize("bits", WIDTHS)
def test_c_sub_ranges_of_the_set(contexts, cases, bits):
    """(3, 13) cuts an octet, (8, 16) is exactly one, (15, 17) straddles the two sets, (23, 24) leaves the first set without
    a query of the pass.  The buffer holds exactly q_end - q_begin rows and a guard row behind them."""
    ix = contexts(14, bits)
    Q, M, meta, scores, active = cases("planes", 14, bits, 24)
    load(ix, M, meta)
    G = meta.G
    with Columns(ix, Q, meta) as qs:
        for q0, q1 in ((3, 13), (8, 16), (15, 17), (23, 24)):
            room = np.full((q1 - q0 + 1, G), 0xA5A5A5A5, np.uint32)
            with DevBuf(ix, room.nbytes) as d:
                d.upload(room)
                hip_check(ix._lib.mk_qset_scores(ix._h, qs.h, q0, q1, d.p))
                hip_check(ix._lib.mk_sync(ix._h))
                d.download(room)
            same(room[:-1], scores[q0:q1], meta, ("rows", q0, q1, bits))
            assert (room[-1] == 0xA5A5A5A5).all(), (q0, q1)


# ---- d. windows of rows

def hot_rows_for(P, ld, budget):
    """api.hip: all rows, or a multiple of P / 64 rows that fits the budget"""
    unit = max(1, P // 64)
    return P if P * ld <= budget else min(P, budget // ld // unit * unit)


def stage_rows(P, P_hot, unit):
    """ensure_cold_stage (api_query.hip) for qset_scan's unit of P / 64 rows: a sixteenth of the hot rows, at least a unit"""
    rows = max(unit, P_hot // 16 // unit * unit)
    return min(rows, -(-(P - P_hot) // unit) * unit + unit)


def launches(ix, fn):
    before = ix.stats()["scan_launches"]
    out = fn()
    return out, ix.stats()["scan_launches"] - before


@pytest.mark.parametrize("bits", WIDTHS)
def test_d_windows_of_the_table_kernel(hip, cases, monkeypatch, bits):
    """Three quarters of the rows in host memory: 16,384 rows of 2 KiB under 8 MiB keep rows [0, 4096) in HBM, the others come
    in 48 staged windows of 256 rows -- a launch of the table kernel each, whose counts add up in the score rows; raw, then
    after compress_index() (columns this random gain nothing: pack_cold leaves the rows as they are, the call's answer is
    what tells the rows in host memory)"""
    case = cases("planes", 14, bits, 16)
    Q, M, meta, scores, active = case
    P, ld = meta.P, 2048
    assert -(-meta.G * bits // 8 // 1024) * 1024 == ld
    P_hot = hot_rows_for(P, ld, 8 << 20)
    stage = stage_rows(P, P_hot, P // 64)
    assert (P_hot, stage) == (4096, 256) and P_hot % 16 == 0 and stage % 16 == 0
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "8")             # (read when the context is made)
    ix = new_context(hip, 14, bits)
    try:
        _, n = launches(ix, lambda: run_case(ix, case, ("windows", bits, "raw")))
        assert n == 2 * (1 + (P - P_hot) // stage)               # (per window: the sparse kernel's zero rows, then the dense launch)
        raw, packed = ix.compress_index()
        assert raw == (P - P_hot) * ld
        run_case(ix, case, ("windows", bits, "after compress_index"))
    finally:
        ix.close()


@pytest.mark.parametrize("bits", WIDTHS)
def test_d_ragged_windows_of_the_compare_kernel(hip, cases, monkeypatch, bits):
    """512 rows at a pitch of 5 KiB (a reservation of 5,120 one-byte or 2,560 two-byte genomes) under 2 MiB: 2,097,152 / 5,120
    = 409 rows fit, of which hot_rows_for keeps 408 = 51 units of P / 64 = 8 rows -- a multiple of 8, not of 16, beyond the
    compare kernel's spill at 248 rows; ensure_cold_stage gives windows of 408 / 16 = 25 -> 24 rows: the launches are rows
    [0, 408), four windows of 24 and one of 8, none a multiple of 16 -- every one takes scan_dense_kernel."""
    case = cases("spill", bits)
    Q, M, meta, scores, active = case
    P, ld, reserve = 512, 5120, 5120 * 8 // bits
    assert P == meta.P and -(-reserve * bits // 8 // 1024) * 1024 == ld and meta.G <= reserve
    P_hot = hot_rows_for(P, ld, 2 << 20)
    stage = stage_rows(P, P_hot, P // 64)
    assert (P_hot, stage) == (408, 24) and P_hot % 8 == 0 and P_hot % 16 != 0 and P_hot > 248
    windows = [(0, P_hot)] + [(r, min(r + stage, P)) for r in range(P_hot, P, stage)]
    assert len(windows) == 6 and all((hi - lo) % 16 for lo, hi in windows)
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "2")
    ix = new_context(hip, 9, bits)
    try:
        ix.reserve(reserve)
        _, n = launches(ix, lambda: run_case(ix, case, ("spill", bits)))
        assert n == 2 * len(windows)                             # (what the library made of the same figures)
        raw, packed = ix.compress_index()
        assert raw == (P - P_hot) * ld
        run_case(ix, case, ("spill", bits, "after compress_index"))
    finally:
        ix.close()


# ---- e. from the index

def test_e_columns_of_the_index_as_queries(contexts, cases):
    """mk_qset_from_index on the planes index: ids [0, 64) -- the 16-byte gather over 16,384 rows -- and 16 scattered ids.  A
    genome's count against itself is its sketch size: up to 16,368 per chunk on every steered and random column"""
    ix = contexts(14, 8)
    Q, M, meta, _, _ = cases("planes", 14, 8, 16)
    load(ix, M, meta)
    ss = (M != meta.empty).sum(0)
    T, G = meta.tile, meta.G
    for ids in (np.arange(64), np.array([G - 1, 0, T, 3, T - 1, 17, 2, 1, 16, T + 1, 500, 21, 26, 31, G - 2, 0])):
        want, active, _ = dl.count(M[:, ids], M, meta.empty)
        with QSet(ix, ids) as qs:
            got = qs.scores()
            np.testing.assert_array_equal(got.astype(np.int64), want)
            np.testing.assert_array_equal(qs.active().astype(np.int64), ss[ids])
            np.testing.assert_array_equal(active, ss[ids])
            np.testing.assert_array_equal(got[np.arange(len(ids)), ids], qs.active())
