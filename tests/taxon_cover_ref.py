"""The yardstick of the taxon-cover tests (tests/test_taxon_cover_definition.py, tests/test_gpu_taxon_cover.py,
tests/test_gpu_cli_taxon_cover.py): per node of a taxonomy the distinct (partition, value) cells its genomes hold and those of
them the sample has seen, from cover_ref's seen and stored -- the oracle's gated sketches and columns -- and lca_ref's Tree, the
distinct values of a row segment taken by sort and compare; and the bytes of `miekki -U`.  Nothing here touches the code under
test."""
import numpy as np

import cover_ref as cr


def node_cover(o, seen_table, fps, nodes):
    """uint64 [n_nodes, 2]: held, covered per node (lo, hi) of `nodes`"""
    empty, rows = cr.empty_of(o), np.arange(o.P)[:, None]
    out = np.zeros((len(nodes), 2), np.uint64)
    for n, (lo, hi) in enumerate(nodes):
        seg = np.sort(fps[:, lo:hi], axis=1)
        first = np.ones(seg.shape, bool)
        first[:, 1:] = seg[:, 1:] != seg[:, :-1]                           # a value counts where it first appears in its row
        first &= seg != empty
        out[n] = int(first.sum()), int((first & seen_table[rows, seg]).sum())
    return out


def outside_children(tree, n):
    """the genomes of node n that lie in none of its children"""
    lo, hi = tree.nodes[n]
    inside = np.zeros(hi - lo, bool)
    for v in range(tree.n):
        if tree.parent[v] == n:
            inside[tree.nodes[v][0] - lo:tree.nodes[v][1] - lo] = True
    return [lo + int(g) for g in np.nonzero(~inside)[0]]


def format_taxon_cover(nc, tree, names):
    """the bytes of `miekki -U`: a line per node with covered > 0, in node order: node, depth, first id, last id, covered, held,
    name"""
    return b"".join(b"%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (v, tree.depth[v], tree.nodes[v][0], tree.nodes[v][1] - 1, int(nc[v][1]), int(nc[v][0]),
                                                   names[v].encode())
                    for v in range(tree.n) if int(nc[v][1]))


def summary_line(n_queries, cells, h, fp_bits, nc):
    nc = np.asarray(nc).reshape(-1, 2)
    return b"taxon cover: %d queries, %d of %d cells seen, %d of %d nodes covered" % (
        n_queries, int(cells), 1 << (h + fp_bits), int((nc[:, 1] > 0).sum()), len(nc))
