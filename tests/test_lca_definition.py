"""The lowest-common-ancestor placement's definition on the oracle alone (tests/lca_ref.py): the four identities the header
states, against clade_ref and tally_ref, and the conditions without which the GPU tests would mean little -- reads at several
depths, on inner nodes, moved by the margin, above a forest.  No GPU, nothing of the code under test."""
import numpy as np
import pytest

import clade_ref as cr
import lca_ref as lr
import tally_ref as tr

THRESHOLDS = [(10, 10.0), (10, 60.0)]
G = 1101


@pytest.fixture(scope="module")
def trees():
    return {name: lr.Tree(nodes, G) for name, nodes in lr.taxonomies(G).items()}


@pytest.fixture(scope="module")
def lists():
    """the oracle's lists of both inputs: tally_ref.Sample as it is, and the grouped collection"""
    s, g = tr.Sample(), lr.Grouped()
    return {"sample": {t: cr.per_query(s.o, s.rows, *t) for t in THRESHOLDS}, "grouped": {t: cr.per_query(g.o, g.rows, *t) for t in THRESHOLDS}}


def test_derivation(trees):
    deep = trees["deep"]
    at = {n: v for v, n in enumerate(deep.nodes)}
    assert deep.nodes[0] == (0, G) and deep.parent[0] is None
    chain = [(256, 257), (254, 259), (250, 520), (100, 1050), (0, G)]
    for child, par in zip(chain, chain[1:]):
        assert deep.parent[at[child]] == at[par]
    assert [deep.depth[at[n]] for n in chain] == [4, 3, 2, 1, 0]
    assert deep.parent[at[(510, 514)]] == at[(250, 520)] and deep.parent[at[(4, 6)]] == 0
    assert deep.parent[at[(1049, 1050)]] == at[(100, 1050)] and deep.parent[at[(1050, 1051)]] == 0
    assert deep.leaf[256] == at[(256, 257)] and deep.leaf[255] == deep.leaf[257] == at[(254, 259)] and deep.leaf[3] == 0 and deep.leaf[5] == at[(4, 6)]
    masked = trees["masked"]
    assert all(l is None for l in masked.leaf[:100]) and all(l is not None for l in masked.leaf[100:])
    assert sum(p is None for p in masked.parent) == 1 + 51                   # several roots
    flat = trees["flat"]
    assert all(p is None for p in flat.parent) and flat.leaf == cr.layouts(G)["fine"]
    single = trees["single"]
    assert single.leaf == list(range(1, G + 1)) and single.parent == [None] + [0] * G
    empty = trees["empty"]
    assert empty.n == 0 and empty.leaf == [None] * G
    # a climb on numbers small enough to follow by hand
    t = lr.Tree([(0, 10), (0, 4), (1, 2), (6, 8)], 12)
    hit = lambda g, x=50.0: (g, 20, x)
    assert t.place([hit(1)], 100)[0] == 2 and t.place([hit(1), hit(3)], 100)[0] == 1 and t.place([hit(1), hit(7)], 100)[0] == 0
    assert t.place([hit(1), hit(11)], 100) == (2, 20, 1)                    # (genome 11 is left out)
    assert t.place([hit(10), hit(11)], 100) == (None, 0, 0)
    assert t.place([hit(1), hit(7, 45.0)], 10)[0] == 0 and t.place([hit(1), hit(7, 44.9)], 10) == (2, 20, 1)
    assert t.place([hit(1), hit(7, 50.0)], 0) == (0, 20, 2)                 # margin 0 keeps the ties
    two = lr.Tree([(0, 4), (6, 8)], 12)
    assert two.place([hit(1), hit(7)], 100) == (lr.ABOVE, 20, 2)


def test_non_vacuity_on_the_oracle_alone(lists, trees):
    """at (10, 10.0) on the grouped collection: no cut had to be moved"""
    per = lists["grouped"][10, 10.0]
    deep, flat = trees["deep"], trees["flat"]
    by_margin = {m: lr.lca_tally(per, deep, m) for m in lr.MARGINS}
    has_child = {p for p in deep.parent if p is not None}
    for m in (0, 10):
        t, _ = by_margin[m]
        depths = {deep.depth[v] for v in range(deep.n) if t[v, 0]}
        assert len(depths) >= 4, (m, depths)
        inner = [v for v in range(deep.n) if t[v, 0] and deep.parent[v] is not None and v in has_child]
        assert inner, m
    # (at margin 100 and these thresholds the chance hits of 8-bit fingerprints drag all but a handful of reads to the root:
    # what the margin is for.  The walk over whole lists is exercised there, the climb's depths at the smaller margins.)
    assert by_margin[100][0][0, 0] > 500
    assert any(len({int(by_margin[m][1][q]) for m in lr.MARGINS}) > 1 for q in range(len(per)))
    assert lr.lca_tally(per, flat, 100)[0][flat.n, 0] > 0
    # masked: some read's only hits are left out, and some read has hits on both sides
    masked = trees["masked"]
    assert any(listed and masked.place(listed, 100)[0] is None for listed in lists["grouped"][10, 60.0])   # (at 10.0 every read has a chance hit beyond 100)
    assert any(0 < sum(masked.leaf[h[0]] is not None for h in listed) < len(listed) for listed in per)
    # tally_ref.Sample: the planted relatives lie far apart, so many reads climb to the root
    t, _ = lr.lca_tally(lists["sample"][10, 10.0], deep, 100)
    assert t[0, 0] > 50


@pytest.mark.parametrize("which", ["sample", "grouped"])
@pytest.mark.parametrize("ms,mi", THRESHOLDS)
def test_identities_on_the_references_own_numbers(lists, trees, which, ms, mi):
    per = lists[which][ms, mi]
    # a forest of disjoint roots that are a clade map's runs, m = 100
    flat = trees["flat"]
    fine = cr.layouts(G)["fine"]
    clades = cr.clade_tally(per, fine)
    t, _ = lr.lca_tally(per, flat, 100)
    np.testing.assert_array_equal(t[:flat.n, 0], clades[:, 1])
    assert t[flat.n, 0] == clades[:, 2].sum() - clades[:, 1].sum()
    # a root with singleton leaves, m = 100
    single = trees["single"]
    plain = cr.plain_tally(per, G)
    t, _ = lr.lca_tally(per, single, 100)
    np.testing.assert_array_equal(t[1:G + 1, 0], plain[:, 1])
    assert t[G + 1, 0] == 0 and t[0, 0] == plain[:, 2].sum() - plain[:, 1].sum()
    # all slots, any taxonomy and margin; monotony in the margin
    for name, tree in trees.items():
        has_leaf = cr.clade_tally(per, tree.has_leaf_map())
        best = int(has_leaf[:, 2].sum()) if len(has_leaf) else 0
        nodes = {}
        for m in lr.MARGINS:
            t, nodes[m] = lr.lca_tally(per, tree, m)
            assert int(t[:, 0].sum()) == best, (name, m)
            assert int(t[:, 2].sum()) <= (int(has_leaf[:, 4].sum()) if len(has_leaf) else 0)
        for q in range(len(per)):
            small, mid, large = (int(nodes[m][q]) for m in lr.MARGINS)
            assert (small == lr.NO_NODE) == (mid == lr.NO_NODE) == (large == lr.NO_NODE)
            if small != lr.NO_NODE:
                assert tree.is_ancestor_or_self(mid, small) and tree.is_ancestor_or_self(large, mid), (name, q)


def test_files_and_lines(trees):
    t = lr.Tree([(0, 10), (0, 4), (1, 2), (6, 8)], 12)
    names = ["root", "", "one leaf", "far"]
    text = lr.taxonomy_file(t.nodes, names)
    assert text == b"# first_id last_id name\n0 9 root\n\n0\t3\n1 1 one leaf\n6\t7\tfar\n"
    counts = np.array([[1, 20, 3], [0, 0, 0], [2, 50, 2], [0, 0, 0], [4, 90, 9]], np.uint64)
    assert lr.format_report(counts, t, names) == b"0\t0\t0\t9\t3\t1\t20\t3\troot\n1\t1\t0\t3\t2\t0\t0\t0\t\n2\t2\t1\t1\t2\t2\t50\t2\tone leaf\n"
    assert lr.format_reads(np.array([2, lr.ABOVE, lr.NO_NODE, 0], np.uint32)) == b"0\t2\n1\t*\n2\t-\n3\t0\n"
    assert lr.summary_line(counts, 9, 10) == b"lca: 9 queries, 7 assigned, 4 above every node, 2 nodes with reads, margin 10"
