"""tests/markers_ref.py, the yardstick of the marker tests, against the definition's identities, without a GPU: on
lca_ref.Grouped() at 8 and 16 bits under every layout of lca_ref.taxonomies() -- the sums against taxon_cover_ref's held and
winners_ref's claimed, the subtree sums against taxon_cover_ref node by node, the singletons against sketch_size, the
all-ones, all-zero and missing tables, and for every node of `deep` and `masked` a count made without minimum, maximum or
climb.  Non-degeneracy is asserted, not assumed.  This file passes without the feature: it proves the inputs and the
yardstick, not the device."""
import numpy as np
import pytest

import cover_ref as cr
import lca_ref as lr
import markers_ref as mr
import taxon_cover_ref as tcr
import winners_ref as wr

G = 1101
LAYOUTS = ["flat", "deep", "masked", "single", "empty"]


class Made:
    def __init__(self, bits):
        self.s = s = lr.Grouped(fp_bits=bits)
        self.o, self.empty = s.o, cr.empty_of(s.o)
        self.fps = cr.stored(s.o)
        self.seen = cr.seen(s.o, s.queries)
        self.trees = {name: lr.Tree(nodes, G) for name, nodes in lr.taxonomies(G).items()}
        self.nm = {name: mr.node_markers(self.fps, self.empty, self.seen, t) for name, t in self.trees.items()}
        self.held_cells = len(np.unique(np.nonzero(self.fps != self.empty)[0] * (self.empty + 1) + self.fps[self.fps != self.empty]))


@pytest.fixture(scope="module", params=[8, 16])
def made(request):
    return Made(request.param)


def test_sums_over_all_slots(made):
    """sum of specific = the distinct held cells of the genomes with a leaf (one root: taxon cover's held(root), above 0); every
    genome with a leaf: sum of covered = the winners' claimed"""
    m = made
    cov = cr.covered(m.o, m.seen, m.fps)
    claimed = wr.won(m.o, m.seen, m.fps, wr.order(cov, m.o.sketch_size))[1]
    for name in ("deep", "single", "flat"):                                # every genome has a leaf
        nm = m.nm[name]
        assert int(nm[:, 0].sum()) == m.held_cells, name
        assert int(nm[:, 1].sum()) == claimed, name
    for name in ("deep", "single"):
        root = tcr.node_cover(m.o, m.seen, m.fps, [(0, G)])[0]
        assert int(m.nm[name][:, 0].sum()) == int(root[0]) and int(m.nm[name][:, 1].sum()) == int(root[1])
        assert not m.nm[name][-1].any()                                    # nothing above a root over everything
    t = m.trees["masked"]
    has = np.array([l is not None for l in t.leaf])
    sub = m.fps[:, has]
    p = np.nonzero(sub != m.empty)[0]
    assert int(m.nm["masked"][:, 0].sum()) == len(np.unique(p * (m.empty + 1) + sub[sub != m.empty]))
    assert m.nm["empty"].shape == (1, 2) and not m.nm["empty"].any()


@pytest.mark.parametrize("name", LAYOUTS)
def test_subtree_sums_against_the_taxon_cover(made, name):
    """clade_specific(n) <= held(n), clade_covered(n) <= covered(n); equalities for a root when no genome outside has a leaf"""
    m = made
    t, nm = m.trees[name], m.nm[name]
    if not t.n:
        return
    clade = mr.clade_sums(nm, t)
    nc = tcr.node_cover(m.o, m.seen, m.fps, t.nodes)
    assert (clade[:, 0] <= nc[:, 0]).all() and (clade[:, 1] <= nc[:, 1]).all()
    assert (nm[:, 1] <= nm[:, 0]).all()
    if name in ("deep", "single"):
        np.testing.assert_array_equal(clade[0], nc[0])
        assert (clade[1:, 0] < nc[1:, 0]).any()                            # ... and strict below it: cells shared with the outside


@pytest.mark.parametrize("name", ["deep", "masked"])
def test_the_count_without_minimum_and_maximum(made, name):
    m = made
    t = m.trees[name]
    clade = mr.clade_sums(m.nm[name], t)
    for n in range(t.n):
        assert tuple(int(x) for x in clade[n]) == mr.inside_not_outside(m.fps, m.empty, m.seen, t, n), (name, n)


def test_singleton_leaves(made):
    m = made
    nm = m.nm["single"]
    assert (nm[1:-1, 0] <= m.o.sketch_size).all() and (nm[1:-1, 0] < m.o.sketch_size).any()
    # an index of one genome: all its cells are its own
    one = lr.Tree([(0, 1)], 1)
    alone = mr.node_markers(m.fps[:, :1], m.empty, m.seen, one)
    assert int(alone[0, 0]) == int(m.o.sketch_size[0]) and int(alone[1, 0]) == 0
    # two identical siblings: their cells are the parent's
    twins = lr.Tree([(0, 2), (0, 1), (1, 2)], 2)
    nm2 = mr.node_markers(m.fps[:, [7, 7]], m.empty, m.seen, twins)
    assert int(nm2[0, 0]) == int(m.o.sketch_size[7]) > 0 and not nm2[1:, 0].any()


def test_tables(made):
    """all ones: covered = specific; all zeros or no table: covered = 0; specific depends on the index and the taxonomy only"""
    m = made
    t, nm = m.trees["deep"], m.nm["deep"]
    ones = mr.node_markers(m.fps, m.empty, np.ones_like(m.seen), t)
    np.testing.assert_array_equal(ones[:, 0], ones[:, 1])
    np.testing.assert_array_equal(ones[:, 0], nm[:, 0])
    for table in (np.zeros_like(m.seen), None):
        zero = mr.node_markers(m.fps, m.empty, table, t)
        np.testing.assert_array_equal(zero[:, 0], nm[:, 0])
        assert not zero[:, 1].any()


def test_non_degeneracy(made):
    m = made
    assert int((m.nm["deep"][:-1, 0] > 0).sum()) >= 100 and m.trees["deep"].n == 108
    assert int(m.nm["flat"][-1, 0]) > 0 and int(m.nm["masked"][-1, 0]) > 0
    assert int(m.nm["single"][-1, 0]) == 0
    assert 0 < int(m.nm["deep"][:, 1].sum()) < int(m.nm["deep"][:, 0].sum())
    assert int(m.nm["flat"][-1, 1]) > 0                                    # covered cells above every node as well


def test_left_out_genomes_do_not_move_an_owner():
    """a value held by two genomes of one node and by a genome inside no node belongs to the node"""
    tree = lr.Tree([(2, 6), (2, 4)], 8)
    fps = np.full((2, 8), 255, np.int64)
    fps[0, [0, 2, 3, 7]] = 9                                                # 0 and 7 have no leaf
    fps[1, [2, 5]] = 9
    nm = mr.node_markers(fps, 255, None, tree)
    np.testing.assert_array_equal(nm[:, 0], [1, 1, 0])


def test_the_command_line_bytes():
    nodes = [(0, 10), (2, 4), (7, 8)]
    tree = lr.Tree(nodes, 10)
    nm = np.array([[50, 0], [20, 0], [10, 3], [7, 2]], np.uint64)
    assert mr.format_markers(nm, tree, ["root", "", "a b"]) == b"0\t0\t0\t9\t3\t80\t0\t50\troot\n2\t1\t7\t7\t3\t10\t3\t10\ta b\n"
    assert mr.summary_line(5, nm, tree) == b"markers: 5 queries, 3 of 80 specific cells covered, 2 of 3 nodes covered, 2 of 7 cells above every node"
