"""The packed counters of the sparse scans AT their limits, whole score rows compared, on every schedule.

Every scan counts mismatches in packed counters (four 8-bit ones per word at one-byte fingerprints, two 16-bit ones at two
bytes); what keeps a counter from passing 255 and carrying into the neighbouring genome's byte is a handful of limits:
the range table's eligibility check (split_kernel), the pieces by count of small sets (qset_prepare_slab), the plain
kernel's widening every 255 entries (scan_item), the unwidened sums of the group kernel, and the byte-wise sums of the S
partials in the selection and in the lists.  The inputs (scan_limits.py, proven by test_scan_limit_inputs.py) put exactly
255 and 256 entries where those limits are, with a genome that matches every entry (counter 0x00) next to genomes that
match none (0xff) at each byte position of a word.

There is no tolerance in this module: everything is compared with the oracle by exact equality.  Two probes per case:
  * whole rows through the partials: query_list(queries, None, min_score=1, min_intersection=0) returns every genome with a
    non-zero score -- its (genome, matches) pairs must be the non-zero entries of the oracle's row, its order, jaccard and
    intersection filter_results' own;
  * the selection: query(queries, 10, ...) equals filter_results; for a steered query once more with min_score = active
    (exactly the copies remain) and active + 1 (nothing).
Which schedule ran is asserted from the context's counters.

Two-byte fingerprints: the 65,535 limit cannot be reached by a short query (at most 4,096 k-mers), so no case pretends to
test it; the two-byte case runs the same 255-entry inputs through the 16-bit lanes.  Likewise the eight-range sums of the
selection cannot overflow while the host keeps S x 178 >= k-mers: no case for that either.

Wall time of the module on an MI355X: about 16 s, most of it the oracle's side of the 13,318-genome collection."""
import struct

import numpy as np
import pytest

import scan_limits as sl

pytestmark = pytest.mark.gpu

GROUP_RUNS = [("0", "10"), ("16", "10"), ("16", "6"), ("16", "4")]       # (MIEKKI_SCAN_GROUPS, MIEKKI_GROUP_WINDOW)


def make_index(c):
    import miekki_amd
    ix = miekki_amd.Miekki(c.k, c.h, c.fpb, sl.BLOOM_LOG2, sl.THRESHOLD)
    ix.reserve(c.G)
    for i in range(0, c.G, 64):
        ix.insert_sequences(c.genomes[i:i + 64])
    assert ix.index_size == c.G
    return ix


@pytest.fixture(scope="module")
def built():
    made = {}

    def get(name):
        if name not in made:
            c = sl.collection(name)
            made[name] = (c, make_index(c))
        return made[name]
    yield get
    for _, ix in made.values():
        ix.close()


def bits(h):
    return (int(h[0]), int(h[1]), struct.pack("<dd", h[2], h[3]))


def launches(ix, fn):
    before = ix.stats()
    out = fn()
    after = ix.stats()
    return out, after["scan_launches"] - before["scan_launches"], after["scan_slab_launches"] - before["scan_slab_launches"]


def assert_schedule(n, slab, want_slab, staged=False, replays=False):
    """replays: mk_query may answer a query with more heap entrants than a device row holds from a dense row of its own"""
    if not want_slab:
        assert slab == 0 and n > 0, (n, slab)
    elif staged:
        assert slab > 0 and n >= 2 * slab, (n, slab)      # one launch over the ranges in HBM, then the staged ranges
    else:
        assert slab > 0 and (n >= slab if replays else n == slab), (n, slab)


def probe(ix, c, qs, rows, steered=None, slab=True, staged=False, tag=""):
    """Both probes of the module's docstring for the set `qs` (rows: the oracle's); returns what the device said."""
    o = c.oracle
    (lists, act), n, ns = launches(ix, lambda: ix.query_list(qs, None, 1, 0.0))
    assert_schedule(n, ns, slab, staged)
    for q, row in enumerate(rows):
        nz = np.flatnonzero(row)
        assert sorted((x.genome, x.matches) for x in lists[q]) == [(int(g), int(row[g])) for g in nz], (tag, "row", q)
        assert [bits(x) for x in lists[q]] == [bits(w) for w in o.filter_results(row, c.G, 1, 0.0)], (tag, "list", q)
    (hits, act2), n, ns = launches(ix, lambda: ix.query(qs, 10, 2, 1.0))
    assert_schedule(n, ns, slab, staged, replays=True)
    for q, row in enumerate(rows):
        assert [bits(x) for x in hits[q]] == [bits(w) for w in o.filter_results(row, 10, 2, 1.0)], (tag, "hits", q)
    np.testing.assert_array_equal(act, act2)
    out = [lists, hits, np.asarray(act).copy()]
    for at, s in sorted((steered or {}).items()):
        assert int(act[at]) == s.active, (tag, at)
        for ms, left in ((s.active, sorted(s.ids)), (s.active + 1, [])):
            got, _ = ix.query(qs, 10, ms, 0.0)
            for q, row in enumerate(rows):
                assert [bits(x) for x in got[q]] == [bits(w) for w in o.filter_results(row, 10, ms, 0.0)], (tag, "min_score", ms, q)
            assert sorted(x.genome for x in got[at]) == left, (tag, at, ms)
            out.append(got)
    return out


def slab_knobs(monkeypatch, groups="16", window="10"):
    monkeypatch.setenv("MIEKKI_SLAB_MIN_QUERIES", "1")
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "1")
    monkeypatch.setenv("MIEKKI_SCAN_GROUPS", groups)
    monkeypatch.setenv("MIEKKI_GROUP_WINDOW", window)


@pytest.mark.parametrize("name", ["h12", "h14", "w16"])
def test_a_range_table_at_255(built, monkeypatch, name):
    """h12: S = 4; h14: S = 16, the selection's tail loop beyond eight ranges; w16: two-byte fingerprints at S = 16."""
    c, ix = built(name)
    qs, where = sl.set_a(c)
    rows = c.oracle.query_sequences(qs)
    runs = []
    for groups, window in GROUP_RUNS:
        slab_knobs(monkeypatch, groups, window)
        runs.append(probe(ix, c, qs, rows, where, tag=(name, groups, window)))
    for r in runs[1:]:
        assert r[:2] == runs[0][:2] and r[3:] == runs[0][3:]
        np.testing.assert_array_equal(r[2], runs[0][2])


@pytest.mark.parametrize("name", ["h12", "h14"])
@pytest.mark.parametrize("groups", ["16", "0"])
def test_b_range_table_refused_at_256(built, monkeypatch, name, groups):
    """One (query, range) of 256 entries: the eligibility check must refuse the range table -- the set falls back to the
    plain schedule (whose kernel widens at 255: case d's limit on this path) --, and take it again without that query."""
    c, ix = built(name)
    slab_knobs(monkeypatch, groups)
    qa, wa = sl.set_a(c)
    qb, wb = sl.set_b(c)
    probe(ix, c, qb, c.oracle.query_sequences(qb), wb, slab=False, tag=(name, "256"))
    probe(ix, c, qa, c.oracle.query_sequences(qa), {34: wa[34]}, slab=True, tag=(name, "255 again"))


@pytest.mark.parametrize("nk", [255, 256])
def test_c_pieces_by_count_one_piece(built, nk):
    """300 queries on 14 tiles: Sc = 1 from the wave count alone.  255 k-mers: one piece of 255; 256: two of 128."""
    c, ix = built("many")
    qs, at = sl.set_c_count(c, nk)
    s = c.special[0]
    rows = c.oracle.query_sequences(qs)
    assert sorted(np.flatnonzero(rows[at] == nk).tolist()) == sorted(s.ids)
    probe(ix, c, qs, rows, tag=("count", nk))
    for ms, left in ((nk, sorted(s.ids)), (nk + 1, [])):
        got, _ = ix.query(qs, 10, ms, 0.0)
        assert sorted(x.genome for x in got[at]) == left, ms


@pytest.mark.parametrize("nk", [2040, 2041, 4096])
def test_c_pieces_by_count_long(built, nk):
    """A handful of queries: 2,040 k-mers are 8 pieces of 255, 2,041 are 9 of 227, 4,096 (the longest short query) 17 of 241."""
    c, ix = built("h14")
    qs, at = sl.set_c_long(c, nk)
    probe(ix, c, qs, c.oracle.query_sequences(qs), tag=("long", nk))


def test_d_plain_kernel_widens_at_255(built):
    """query_sequences -> mk_query_scores: the plain kernel, dense rows out; 255, 256, 510, 511, 765 entries."""
    c, ix = built("h12")
    qs = sl.set_d(c)
    got, n, ns = launches(ix, lambda: ix.query_sequences(qs))
    assert ns == 0
    np.testing.assert_array_equal(got, c.oracle.query_sequences(qs))
    more = qs + [s.seq for s in c.special]
    np.testing.assert_array_equal(ix.query_sequences(more), c.oracle.query_sequences(more))


@pytest.mark.parametrize("groups", ["16", "0"])
def test_e_staged_cold_ranges(monkeypatch, groups):
    """Case a at S = 4 under a 3 MiB budget: 1,030 genomes are 2 KiB a row, so rows [0, 1536) stay in HBM -- range 0 whole,
    range 1 across the boundary, ranges 2 and 3 in host memory -- and the set holds a 255-entry range in each of them."""
    c = sl.collection("h12")
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "3")               # (read when the context is made)
    slab_knobs(monkeypatch, groups)
    ix = make_index(c)
    try:
        qs, where = sl.set_a(c)
        assert {s.r for s in where.values()} == {0, 1, 2, 3}
        probe(ix, c, qs, c.oracle.query_sequences(qs), where, staged=True, tag=("cold", groups))
    finally:
        ix.close()
