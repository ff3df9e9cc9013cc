"""The inputs of test_gpu_scan_limits.py, proven with the oracle alone before any GPU is involved: the steered queries
hold exactly the planned number of entries per partition range under the built collection's Bloom gate, their copies in
the collection match every entry, and the genomes sharing a counter word with a copy match none.  A constructor that
cannot reach its target fails (scan_limits raises): nothing here skips."""
import numpy as np
import pytest

import scan_limits as sl

NAMES = ["h12", "h14", "w16"]


@pytest.mark.parametrize("name", NAMES)
def test_steered_queries_hold_the_planned_entries_per_range(name):
    c = sl.collection(name)
    o = c.oracle
    assert o.index_size == c.G and c.G % (1024 // c.W) not in (0,), "the last tile must be ragged"
    full_ranges = set()
    for s in c.special:
        if s.r is None:
            continue
        counts = sl.per_range(o, c.S, s.seq)
        _, _, sketched = o.minhash_sketch_partition(s.seq)
        assert counts[s.r] == s.want, (s.tag, counts)
        assert all(n < 255 for r, n in enumerate(counts) if r != s.r), (s.tag, counts)
        assert counts.sum() == s.active == sketched, s.tag                   # every entry passes the gate: active == planned
        assert len(s.seq) - c.k <= c.S * sl.HOST_MEAN, s.tag                 # the host keeps S: S is what MIEKKI_SLAB_MIB gives
        if s.want == 255:
            full_ranges.add(s.r)
    assert 0 in full_ranges and c.S - 1 in full_ranges and any(0 < r < c.S - 1 for r in full_ranges)


@pytest.mark.parametrize("name", NAMES + ["many"])
def test_copies_match_everything_and_their_word_neighbours_nothing(name):
    c = sl.collection(name)
    rows = c.oracle.query_sequences([s.seq for s in c.special])
    for s, row in zip(c.special, rows):
        assert sorted(g % 4 for g in s.ids[:4]) == [0, 1, 2, 3], s.tag      # each byte position of a counter word
        assert any(g >= c.G - c.G % (1024 // c.W) for g in c.special[0].ids)  # and one copy in the ragged last tile
        for g in s.ids:
            assert row[g] == s.active, (s.tag, g)
            for n in range(g & ~3, min((g & ~3) + 4, c.G)):
                assert n == g or row[n] == 0, (s.tag, g, n)
        assert sorted(np.flatnonzero(row == s.active).tolist()) == sorted(s.ids), s.tag
        assert row.max() == s.active


@pytest.mark.parametrize("name", NAMES)
def test_sets_a_and_b(name):
    c = sl.collection(name)
    qs, where = sl.set_a(c)
    assert len(qs) >= 35 and len(qs) % 16 != 0
    assert sorted(where)[:2] == [3, 4] and max(where) == len(qs) - 1         # two neighbours in one group, one the last query
    assert {s.r for s in where.values()} >= {0, c.S - 1} and all(s.want == 255 for s in where.values())
    assert b"" in qs and any(0 < len(q) < c.k for q in qs)
    limit = 255 if c.W == 1 else 65535
    worst = max(int(sl.per_range(c.oracle, c.S, q).max()) for q in qs if len(q) > c.k)
    assert worst == 255 <= limit                                             # the range table holds: at, not beyond, 255
    assert all(len(q) - c.k <= c.S * sl.HOST_MEAN for q in qs)
    if c.W == 1:
        qb, wb = sl.set_b(c)
        assert len(qb) == len(qs) + 1
        assert max(int(sl.per_range(c.oracle, c.S, q).max()) for q in qb if len(q) > c.k) == 256
        assert [q for i, q in enumerate(qb) if i != 10] == qs


def test_pieces_by_count_inputs():
    c = sl.collection("many")
    o = c.oracle
    assert -(-c.G * c.W // 1024) * 300 >= 4096                               # enough (query, tile) waves that Sc is 1
    for nk in (255, 256):
        qs, at = sl.set_c_count(c, nk)
        assert len(qs) == 300 < 512
        ks = [max(len(q) - c.k, 0) for q in qs]
        assert max(ks) == ks[at] == nk and sorted(ks)[-2] < 255
        assert len(sl.gated_partitions(o, qs[at])) == nk == o.query_sequence(qs[at])[1]
    c = sl.collection("h14")
    for nk, pieces, chunk in ((2040, 8, 255), (2041, 9, 227), (4096, 17, 241)):
        qs, at = sl.set_c_long(c, nk)
        ks = [len(q) - c.k for q in qs]
        assert max(ks) == ks[at] == nk
        assert max(8, -(-nk // 255)) == pieces and -(-nk // pieces) == chunk  # qset_prepare_slab's arithmetic for a handful
        entries = len(sl.gated_partitions(c.oracle, qs[at]))
        if nk <= 2041:
            assert entries == nk                                             # every piece is full: 8 x 255, or 9 x 227 less two
        else:
            assert entries > 5 * chunk                                       # several full pieces of 241


def test_plain_kernel_inputs():
    c = sl.collection("h12")
    qs = sl.set_d(c)
    assert [c.oracle.query_sequence(q)[1] for q in qs] == list(sl.D_ENTRIES)
    assert all(len(q) - c.k <= 4096 for q in qs)
    rows = c.oracle.query_sequences(qs)
    # genomes that mismatch EVERY entry (a counter byte of 255 per 255 entries: the very short fillers) next to the
    # genome the queries are cut from
    assert all((row == 0).sum() >= 16 and row.max() > 100 for row in rows)
