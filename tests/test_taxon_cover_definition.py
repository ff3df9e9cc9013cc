"""tests/taxon_cover_ref.py, the yardstick of the taxon-cover tests, against the definition and its identities, without a GPU:
on lca_ref.Grouped() under every layout of lca_ref.taxonomies() -- a brute-force count over sets of tuples on `deep`, the
singletons against cover_ref.covered and sketch_size, the root against winners_ref's claimed, the bounds between a node and
its children, the all-ones and all-zero tables."""
import numpy as np
import pytest

import cover_ref as cr
import lca_ref as lr
import taxon_cover_ref as tcr
import winners_ref as wr

G = 1101


@pytest.fixture(scope="module")
def grouped():
    s = lr.Grouped()
    s.fps = cr.stored(s.o)
    s.seen = cr.seen(s.o, s.queries)
    s.cov = cr.covered(s.o, s.seen, s.fps)
    s.trees = {name: lr.Tree(nodes, G) for name, nodes in lr.taxonomies(G).items()}
    s.nc = {name: tcr.node_cover(s.o, s.seen, s.fps, t.nodes) for name, t in s.trees.items()}
    return s


def brute(o, seen_table, fps, lo, hi):
    """(held, covered) of [lo, hi) from the definition: the set of (p, v) over the node's genomes"""
    empty = cr.empty_of(o)
    cells = {(p, int(fps[p, g])) for p in range(o.P) for g in range(lo, hi) if fps[p, g] != empty}
    return len(cells), sum(1 for p, v in cells if seen_table[p, v])


def test_the_yardstick_is_the_definition(grouped):
    s = grouped
    for v, (lo, hi) in enumerate(s.trees["deep"].nodes):
        if hi - lo <= 300:                                                 # (the wide nodes by the bounds below)
            assert tuple(int(x) for x in s.nc["deep"][v]) == brute(s.o, s.seen, s.fps, lo, hi), (lo, hi)
    assert tuple(int(x) for x in s.nc["deep"][0]) == brute(s.o, s.seen, s.fps, 0, G)


def test_singletons_are_the_plain_count(grouped):
    s = grouped
    nc = s.nc["single"]
    np.testing.assert_array_equal(nc[1:, 0], s.o.sketch_size)
    np.testing.assert_array_equal(nc[1:, 1], s.cov)
    assert nc[1:, 1].any() and (nc[1:, 1] < nc[1:, 0]).any()


def test_the_root_is_the_winners_claimed(grouped):
    s = grouped
    claimed = wr.won(s.o, s.seen, s.fps, wr.order(s.cov, s.o.sketch_size))[1]
    for name in ("deep", "single"):
        assert int(s.nc[name][0, 1]) == claimed
    assert 0 < claimed < int(s.seen.sum())                                 # some seen cells nobody holds
    # ... and below the sum of the genomes' counts: shared cells count once
    assert claimed < int(s.cov.sum()) and int(s.nc["single"][0, 0]) < int(s.o.sketch_size.sum())


@pytest.mark.parametrize("name", ["flat", "deep", "masked", "single"])
def test_a_node_lies_between_its_children(grouped, name):
    """max over children <= value(n) <= sum over children + the same count over the node's genomes in no child"""
    s = grouped
    t, nc = s.trees[name], s.nc[name]
    assert (nc[:, 1] <= nc[:, 0]).all()
    for n in range(t.n):
        kids = [v for v in range(t.n) if t.parent[v] == n]
        if not kids:
            continue
        rest = tcr.outside_children(t, n)
        alone = tcr.node_cover(s.o, s.seen, s.fps, [(g, g + 1) for g in rest]).sum(0) if rest else np.zeros(2, np.uint64)
        for col in (0, 1):
            assert max(int(nc[v, col]) for v in kids) <= int(nc[n, col]) <= sum(int(nc[v, col]) for v in kids) + int(alone[col]), (name, n, col)


def test_all_ones_and_all_zero_tables(grouped):
    s = grouped
    nodes = s.trees["deep"].nodes
    ones = tcr.node_cover(s.o, np.ones_like(s.seen), s.fps, nodes)
    np.testing.assert_array_equal(ones[:, 0], ones[:, 1])
    np.testing.assert_array_equal(ones[:, 0], s.nc["deep"][:, 0])          # held depends on the index and the taxonomy only
    zero = tcr.node_cover(s.o, np.zeros_like(s.seen), s.fps, nodes)
    np.testing.assert_array_equal(zero[:, 0], s.nc["deep"][:, 0])
    assert not zero[:, 1].any()
    assert tcr.node_cover(s.o, s.seen, s.fps, []).shape == (0, 2)


def test_the_command_line_bytes():
    nodes = [(0, 10), (2, 4), (7, 8)]
    tree = lr.Tree(nodes, 10)
    nc = np.array([[50, 9], [20, 0], [10, 10]], np.uint64)
    assert tcr.format_taxon_cover(nc, tree, ["root", "", "a b"]) == b"0\t0\t0\t9\t9\t50\troot\n2\t1\t7\t7\t10\t10\ta b\n"
    assert tcr.summary_line(3, 77, 9, 8, nc) == b"taxon cover: 3 queries, 77 of 131072 cells seen, 2 of 3 nodes covered"
