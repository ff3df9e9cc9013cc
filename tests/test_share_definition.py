"""The abundance estimate's definition on the oracle alone (tests/share_ref.py): the consequences the header states -- the sum
bounds, R = 1 as the equal split, the three identities with the plain tally at margin 100, independence of the lists' order and
of how the queries are cut -- a two-strain case small enough to follow by hand, the starved fallback at shift 32, and the bytes
of `miekki -E`.  And the conditions without which the GPU tests would mean little: the fixtures hold settled, shared and
unassigned reads, lists longer than a wave, and reads that starve.  No GPU, nothing of the code under test."""
import random

import pytest

import clade_ref as cr
import lca_ref as lr
import share_ref as sr
import tally_ref as tr

THRESHOLDS = [(10, 10.0), (10, 60.0), (10, 150.0)]
G = 1101
ONE = 1 << 32


@pytest.fixture(scope="module")
def lists():
    """the oracle's lists of both inputs: tally_ref.Sample as it is, and the grouped collection"""
    s, g = tr.Sample(), lr.Grouped()
    return {"sample": {t: cr.per_query(s.o, s.rows, *t) for t in THRESHOLDS}, "grouped": {t: cr.per_query(g.o, g.rows, *t) for t in THRESHOLDS}}


def test_margin_rule_by_hand():
    hit = lambda g, x: (g, 20, x)
    assert sr.kept([], 100) == ()
    assert sr.kept([hit(3, 50.0)], 0) == (3,)
    assert sr.kept([hit(1, 50.0), hit(7, 45.0), hit(9, 44.9)], 10) == (1, 7)
    assert sr.kept([hit(1, 50.0), hit(7, 45.0), hit(9, 44.9)], 100) == (1, 7, 9)
    assert sr.kept([hit(1, 50.0), hit(7, 50.0), hit(9, 49.9)], 0) == (1, 7)          # margin 0 keeps the ties
    p = sr.Pool(12).add(()).add((4,)).add((1, 7)).add((1, 7, 9))
    assert p.info() == {"queries": 4, "assigned": 3, "shared_reads": 2, "entries": 5}
    assert p.unique[4] == 1 and p.shared[1] == p.shared[7] == 2 and p.shared[9] == 1 and sum(p.shared) == 5


def test_the_fixtures_hold_every_case(lists):
    """what the issue measured on the oracle's lists: no cut had to be moved"""
    at = lists["sample"][(10, 10.0)]
    p = sr.pool_of(at, 100, G)
    assert (p.settled, len(p.lists), p.entries, max(map(len, p.lists))) == (0, 628, 154_647, 820)
    assert sum(len(l) > 64 for l in p.lists) == 506 and sum(len(l) > 256 for l in p.lists) == 304
    p = sr.pool_of(at, 10, G)
    assert (p.settled, len(p.lists), p.entries, max(map(len, p.lists))) == (573, 55, 167, 18)
    p = sr.pool_of(at, 0, G)
    assert (p.settled, len(p.lists), p.entries) == (628, 0, 0)
    p = sr.pool_of(lists["sample"][(10, 60.0)], 100, G)
    assert (p.settled, len(p.lists)) == (11, 617)
    p = sr.pool_of(lists["grouped"][(10, 60.0)], 100, G)
    assert (p.settled, len(p.lists)) == (15, 613)
    at = lists["sample"][(10, 150.0)]
    assert sr.pool_of(at, 100, G).queries - sr.pool_of(at, 100, G).assigned == 20
    assert len(sr.pool_of(at, 100, G).lists) == 213 and len(sr.pool_of(at, 10, G).lists) == 38


@pytest.mark.parametrize("name", ["sample", "grouped"])
@pytest.mark.parametrize("ms,mi", THRESHOLDS)
def test_identities_with_the_plain_tally(lists, name, ms, mi):
    """at margin 100: unique is the tally's unique, unique + shared its listed, N its sum of best"""
    at = lists[name][ms, mi]
    t = cr.plain_tally(at, G)
    p = sr.pool_of(at, 100, G)
    assert p.unique == [int(x) for x in t[:, 1]]
    assert [u + s for u, s in zip(p.unique, p.shared)] == [int(x) for x in t[:, 0]]
    assert p.assigned == int(t[:, 2].sum())
    assert p.queries == len(at)
    for margin in (0, 10):                                                  # a smaller margin moves reads from shared to settled, never away
        q = sr.pool_of(at, margin, G)
        assert q.assigned == p.assigned and q.settled >= p.settled and q.entries <= p.entries


@pytest.mark.parametrize("margin", sr.MARGINS)
def test_rounds_on_the_fixture(lists, margin):
    """the sum bounds and p < 2^32 (asserted inside share_ref.rounds, every round), R = 1 as the equal split, delta = 0 at
    shift 32 after 25 rounds, and the starved reads of round 25 the issue counted"""
    at = lists["sample"][(10, 10.0)]
    p = sr.pool_of(at, margin, G)
    A, delta, starved, s = sr.rounds(p, 1)
    assert s == (628).bit_length() == 10 and starved == 0
    equal = [u << 32 for u in p.unique]
    for l in p.lists:
        for g in l:
            equal[g] += ONE // len(l)
    assert A == equal and delta == sum(A)
    trace = []
    A, delta, starved, s = sr.rounds(p, 25, 32, trace)
    assert s == 32 and delta == 0 and trace[-1][0] == trace[-2][0] and trace[24] == (A, delta, starved)
    assert trace[1] == sr.rounds(p, 2, 32)[:3]
    assert starved == {100: 8, 10: 3, 0: 0}[margin]
    assert sr.rounds(p, 25)[2] == 0                                         # with the automatic shift: none


def test_starved_counts_on_the_first_500_reads(lists):
    for (ms, mi), want_all, want_few in (((10, 10.0), 8, 121), ((10, 60.0), 6, 23)):
        at = lists["sample"][ms, mi]
        assert sr.rounds(sr.pool_of(at, 100, G), 25, 32)[2] == want_all
        assert sr.rounds(sr.pool_of(at[:500], 100, G), 25, 32)[2] == want_few
        assert sr.rounds(sr.pool_of(at[:500], 100, G), 25)[2] == 0


def test_order_and_cuts_leave_no_trace(lists):
    at = lists["grouped"][(10, 60.0)]
    want = sr.rounds(sr.pool_of(at, 100, G), 7)
    mixed = list(at)
    random.Random(3).shuffle(mixed)
    assert sr.rounds(sr.pool_of(mixed, 100, G), 7) == want
    cut = sr.Pool(G)
    for piece in (at[:211], at[211:500], at[500:]):
        cut.add_queries(piece, 100)
    assert cut.multiset() == sr.pool_of(at, 100, G).multiset() and sr.rounds(cut, 7) == want
    off, ids = sr.pool_of(at, 100, G).offsets_ids()                         # the round trip the GPU tests feed mk_share_add_lists with
    again = sr.Pool(G)
    for i in range(len(off) - 1):
        again.add(ids[int(off[i]):int(off[i + 1])])
    assert again.info() == sr.pool_of(at, 100, G).info() and sr.rounds(again, 7) == want


def test_two_strains():
    """unique reads 30 : 10 and 100 reads that both strains share: the shared split starts at 50 : 50 and moves, round by
    round, towards the 75 : 25 the unique reads state -- and after 50 rounds lies strictly between the two"""
    p = sr.Pool(2)
    for _ in range(30):
        p.add((0,))
    for _ in range(10):
        p.add((1,))
    for _ in range(100):
        p.add((0, 1))
    assert p.assigned == 140 and sr.auto_shift(p) == 8
    trace = []
    A, delta, starved, s = sr.rounds(p, 50, trace=trace)
    share0 = [a[0] - (30 << 32) for a, _, _ in trace]                             # strain 0's part of the 100 shared reads
    assert share0[0] == 50 << 32
    assert all(x < y for x, y in zip(share0, share0[1:5])) and all(x <= y for x, y in zip(share0, share0[1:]))
    assert 50 << 32 < share0[-1] < 75 << 32
    assert (140 << 32) - 200 <= A[0] + A[1] <= 140 << 32 and starved == 0
    assert delta == abs(trace[-1][0][0] - trace[-2][0][0]) + abs(trace[-1][0][1] - trace[-2][0][1])


def test_starved_fallback_at_shift_32():
    """three genomes that only shared reads name: after round 1 every one of them holds less than one read, so at shift 32
    every weight is zero, the read is starved and split evenly; with the automatic shift nothing starves"""
    p = sr.Pool(4).add((0, 1, 2)).add((3,))
    A, delta, starved, s = sr.rounds(p, 2, 32)
    assert starved == 1 and A == [ONE // 3] * 3 + [ONE] and delta == 0
    A, delta, starved, s = sr.rounds(p, 2)
    assert s == 2 and starved == 0 and A[:3] == [ONE // 3] * 3              # p = floor(2^32 / 3) >> 2 each: still the equal split
    with pytest.raises(AssertionError):
        sr.rounds(p, 1, 1)                                                  # below bit_length(N)
    with pytest.raises(AssertionError):
        sr.rounds(p, 1, 33)


def test_file_and_line_formats():
    assert sr.reads_text(0) == b"0.000" and sr.reads_text(ONE) == b"1.000" and sr.reads_text(ONE - 1) == b"0.999"
    assert sr.reads_text((7 << 32) + (ONE >> 1)) == b"7.500" and sr.reads_text((ONE // 3) * 2) == b"0.666"
    assert sr.reads_text((123456789 << 32) + 4294968) == b"123456789.001"
    p = sr.Pool(5).add((0, 2)).add((2,)).add(()).add((0, 2, 4))
    A, delta, _, _ = sr.rounds(p, 1)
    assert sr.format_abundance(A, p.unique, p.shared) == b"0\t0.833\t0\t2\n2\t1.833\t1\t2\n4\t0.333\t0\t1\n"
    assert sr.summary_line(p, 1, 100, delta) == (b"abundance: 4 queries, 3 assigned, 2 shared by several genomes, 5 ids stored, 3 genomes listed, "
                                                 b"1 rounds, margin 100, last change 2.999")
