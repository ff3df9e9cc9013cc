"""The yardstick of the marker tests (tests/test_markers_definition.py, tests/test_markers_abi.py, tests/test_gpu_markers.py,
tests/test_gpu_cli_markers.py): every held cell (partition, value) of the genomes that have a leaf credited to the deepest
node of a taxonomy that contains all its holders, from a matrix of fingerprints (cover_ref.stored over the oracle's columns, or
a crafted one), a table of seen cells (cover_ref.seen) and lca_ref's Tree -- np.minimum.at / np.maximum.at per (row, value),
the climb in Python, the subtree sums, and the bytes of `miekki -V` with its stdout line.  Nothing here touches the code under
test."""
import numpy as np


def holders(fps, empty, tree):
    """(key, a, b) per distinct cell that some genome with a leaf holds: key = p * (empty + 1) + v, a / b = its smallest /
    largest holder with a leaf.  Genomes from tree.G on (appended after the taxonomy was made) are left out."""
    fps = np.asarray(fps, np.int64)[:, :tree.G]
    has = np.array([l is not None for l in tree.leaf], bool)
    p, g = np.nonzero((fps != empty) & has[None, :fps.shape[1]])
    keys, inv = np.unique(p * (empty + 1) + fps[p, g], return_inverse=True)
    a, b = np.full(len(keys), tree.G, np.int64), np.full(len(keys), -1, np.int64)
    np.minimum.at(a, inv, g)
    np.maximum.at(b, inv, g)
    return keys, a, b


def owner_of(tree, a, b):
    """the deepest node that contains genomes a and b: climb from leaf[a] until hi > b; tree.n: above every node"""
    v = tree.leaf[a]
    while v is not None and not tree.nodes[v][1] > b:
        v = tree.parent[v]
    return tree.n if v is None else v


def node_markers(fps, empty, seen_table, tree):
    """uint64 [n_nodes + 1, 2]: specific, covered per node, the last row above every node.  seen_table: bool [P, empty + 1]
    or None (covered = 0)."""
    keys, a, b = holders(fps, empty, tree)
    memo, own = {}, np.zeros(len(keys), np.int64)
    for i, ab in enumerate(zip(a.tolist(), b.tolist())):
        if ab not in memo:
            memo[ab] = owner_of(tree, *ab)
        own[i] = memo[ab]
    out = np.zeros((tree.n + 1, 2), np.uint64)
    out[:, 0] = np.bincount(own, minlength=tree.n + 1)
    if seen_table is not None:
        hit = np.asarray(seen_table, bool).reshape(-1)[keys]
        out[:, 1] = np.bincount(own[hit], minlength=tree.n + 1)
    return out


def clade_sums(nm, tree):
    """uint64 [n_nodes, 2]: a node's counters and those of everything below it (Python integers on the way)"""
    c = [[int(x) for x in row] for row in nm[:tree.n]]
    for v in range(tree.n - 1, -1, -1):
        if tree.parent[v] is not None:
            for k in (0, 1):
                c[tree.parent[v]][k] += c[v][k]
    return np.array(c, np.uint64).reshape(tree.n, 2)


def inside_not_outside(fps, empty, seen_table, tree, n):
    """(clade_specific, clade_covered) of node n without minimum, maximum or climb: the cells held inside [lo, hi) and by no
    genome outside it that has a leaf"""
    fps = np.asarray(fps, np.int64)[:, :tree.G]
    lo, hi = tree.nodes[n]
    has = np.array([l is not None for l in tree.leaf], bool)
    inside = np.zeros(tree.G, bool)
    inside[lo:hi] = True

    def cells(which):
        p, g = np.nonzero((fps != empty) & which[None, :])
        return np.unique(p * (empty + 1) + fps[p, g])
    own = np.setdiff1d(cells(inside), cells(has & ~inside), assume_unique=True)
    return len(own), int(np.asarray(seen_table, bool).reshape(-1)[own].sum())


def format_markers(nm, tree, names):
    """the bytes of `miekki -V`: a line per node whose subtree has a covered cell, in node order: node, depth, first id, last
    id, clade_covered, clade_specific, covered, specific, name"""
    clade = clade_sums(nm, tree)
    return b"".join(b"%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (v, tree.depth[v], tree.nodes[v][0], tree.nodes[v][1] - 1, int(clade[v][1]),
                                                           int(clade[v][0]), int(nm[v][1]), int(nm[v][0]), names[v].encode())
                    for v in range(tree.n) if int(clade[v][1]))


def summary_line(n_queries, nm, tree):
    clade = clade_sums(nm, tree)
    return b"markers: %d queries, %d of %d specific cells covered, %d of %d nodes covered, %d of %d cells above every node" % (
        n_queries, sum(int(r[1]) for r in nm[:tree.n]), sum(int(r[0]) for r in nm[:tree.n]), sum(1 for r in clade if int(r[1])), tree.n,
        int(nm[tree.n][1]), int(nm[tree.n][0]))
