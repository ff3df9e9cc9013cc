"""The yardstick of the hierarchy tests (tests/test_host_hierarchy.py, tests/test_gpu_cli_hierarchy.py): the layout of nested
family labels as `miekki -J -H -O` writes it, stated independently of host/hierarchy.hpp -- a sort by key tuples and a stack of
open families.  Nothing here touches the code under test."""
import numpy as np


def layout(labels):
    """labels[l][j]: the label of genome j at level l, level 0 the loosest, levels nested.
    Returns (order, nodes): order[p] = the old id at place p; nodes = [(first, last, name, depth)] in preorder."""
    labels = np.asarray(labels, np.int64)
    L, G = labels.shape
    order = sorted(range(G), key=lambda j: tuple(int(labels[l, j]) for l in range(L)) + (j,))
    families = []                                    # (level, label, first place, last place), as they close
    open_ = []                                       # the families around the previous place, level 0 first: [label, first place]
    for p, j in enumerate(order):
        key = [int(labels[l, j]) for l in range(L)]
        keep = 0
        while keep < len(open_) and open_[keep][0] == key[keep]:
            keep += 1
        while len(open_) > keep:
            label, first = open_.pop()
            families.append((len(open_), label, first, p - 1))
        for l in range(keep, L):
            open_.append([key[l], p])
    while open_:
        label, first = open_.pop()
        families.append((len(open_), label, first, G - 1))
    span = {(l, label): (first, last) for l, label, first, last in families}
    picked = []
    for l, label, first, last in families:
        if last == first:
            continue                                 # a family of one: its leaf stands for it
        if l and span[(l - 1, int(labels[l - 1, label]))] == (first, last):
            continue                                 # the family of the level above, unchanged: one node, named for the loosest level
        picked.append((first, last, "L%d.%d" % (l, label)))
    picked += [(p, p, "g%d" % j) for p, j in enumerate(order)]
    picked.sort(key=lambda n: (n[0], -n[1]))
    nodes, around = [], []
    for first, last, name in picked:
        while around and around[-1] < first:
            around.pop()
        nodes.append((first, last, name, len(around)))
        around.append(last)
    return order, nodes


def order_bytes(order):
    return b"".join(b"%d\n" % j for j in order)


def taxonomy_bytes(nodes):
    return b"".join(b"%d %d %s\n" % (first, last, name.encode()) for first, last, name, _ in nodes)


def summary_line(labels, nodes):
    labels = np.asarray(labels, np.int64)
    L, G = labels.shape
    counts = b"/".join(b"%d" % int((labels[l] == np.arange(G)).sum()) for l in range(L))
    deepest = max((d + 1 for *_, d in nodes), default=0)
    return b"hierarchy: %d levels, %s families, %d nodes, depth %d" % (L, counts, len(nodes), deepest)


def levels_argument(levels):
    """the -J argument of (min_score, min_intersection) pairs; repr() of a float is a plain decimal at these sizes"""
    return ",".join("%d:%s" % (s, repr(float(mi))) for s, mi in levels)
