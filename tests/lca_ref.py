"""The yardstick of the lowest-common-ancestor tests (tests/test_lca_definition.py, tests/test_gpu_lca.py,
tests/test_gpu_cli_lca.py): per query the oracle's own filter_results through clade_ref.per_query -- the full list with its
intersections -- restricted to the genomes that have a leaf, the margin rule on those intersections in Python floats (IEEE
doubles) with the two products the header writes, the climb up a parent table derived here by plain search, the counters in
Python integers, and the bytes of `miekki -T -y -Y`.  Nothing here touches the code under test."""
import numpy as np

import clade_ref as cr
import families_ref as fr
import synth

COLUMNS = ("reads", "best_matches", "hits")
NO_NODE = 0xffffffff
ABOVE = 0xfffffffe
MARGINS = (0, 10, 100)


# ---- taxonomies: lists of (lo, hi), nested intervals [lo, hi) in preorder ---------------------------------------------------
def preorder(nodes):
    return sorted(nodes, key=lambda n: (n[0], -n[1]))


def taxonomies(G=1101):
    """name -> nodes.  `flat`: clade_ref's `fine` runs as roots (a forest, the above-every-node slot); `deep`: five levels
    around the grouped collection's planted runs, with singleton leaves over the last 101 genomes; `masked`: `deep` without
    its root and without anything over [0, 100) -- left-out genomes, and reads whose only hits are left out; `single`: a root
    and a leaf per genome; `empty`: no node."""
    assert G == 1101
    flat = [(cr.FINE[i], cr.FINE[i + 1]) for i in range(len(cr.FINE) - 1)]
    deep = preorder([(0, G), (100, 1050), (250, 520), (254, 259), (256, 257), (510, 514), (4, 6)] + [(g, g + 1) for g in range(1000, G)])
    masked = [n for n in deep if n != (0, G) and n[0] >= 100]
    single = [(0, G)] + [(g, g + 1) for g in range(G)]
    return {"flat": flat, "deep": deep, "masked": masked, "single": single, "empty": []}


def derive(nodes, G):
    """(parent, leaf, depth) by plain search: parent[v] = the smallest interval that contains node v properly or None,
    leaf[g] = the deepest node that contains genome g or None, depth[v] = the number of v's ancestors"""
    for lo, hi in nodes:
        assert 0 <= lo < hi <= G
    assert len(set(nodes)) == len(nodes) and list(nodes) == preorder(nodes)
    for a in nodes:
        for b in nodes:
            apart = a[1] <= b[0] or b[1] <= a[0]
            inside = (a[0] <= b[0] and b[1] <= a[1]) or (b[0] <= a[0] and a[1] <= b[1])
            assert apart or inside, (a, b)
    parent = []
    for v, (lo, hi) in enumerate(nodes):
        around = [u for u, (l, h) in enumerate(nodes) if u != v and l <= lo and hi <= h]
        parent.append(min(around, key=lambda u: nodes[u][1] - nodes[u][0]) if around else None)
    depth = []
    for v in range(len(nodes)):
        d, u = 0, parent[v]
        while u is not None:
            d, u = d + 1, parent[u]
        depth.append(d)
    leaf = [None] * G
    size = [None] * G
    for v, (lo, hi) in enumerate(nodes):
        for g in range(lo, hi):
            if size[g] is None or hi - lo < size[g]:
                leaf[g], size[g] = v, hi - lo
    return parent, leaf, depth


class Tree:
    def __init__(self, nodes, G):
        self.nodes, self.G = list(nodes), G
        self.parent, self.leaf, self.depth = derive(self.nodes, G)
        self.n = len(self.nodes)

    def has_leaf_map(self):
        """the clade map "has a leaf / left out" """
        return [0 if l is not None else None for l in self.leaf]

    def is_ancestor_or_self(self, up, v):
        """node `up` (or ABOVE) is v or lies above it"""
        if up == ABOVE:
            return True
        if v == ABOVE:
            return False
        while v is not None:
            if v == up:
                return True
            v = self.parent[v]
        return False

    def place(self, listed, margin):
        """(node, matches of best', |L''|) of a query whose list (clade_ref.per_query) is `listed`; node None: unassigned,
        ABOVE: above every node"""
        mine = [h for h in listed if self.leaf[h[0]] is not None]
        if not mine:
            return None, 0, 0
        best = cr.best_of(mine)
        x = best[2]
        kept = [h for h in mine if h[2] * 100.0 >= x * float(100 - margin)]
        a, b = min(h[0] for h in kept), max(h[0] for h in kept)
        v = self.leaf[a]
        while v is not None and not self.nodes[v][1] > b:
            v = self.parent[v]
        return (ABOVE if v is None else v), best[1], len(kept)


def lca_tally(lists, tree, margin):
    """(uint64 [n_nodes + 1, 3]: reads, best_matches, hits per node, the last row above every node; uint32 [queries]: each
    query's node, ABOVE or NO_NODE) over the queries whose lists (clade_ref.per_query) are `lists`, in Python integers"""
    t = [[0, 0, 0] for _ in range(tree.n + 1)]
    per_read = []
    for listed in lists:
        v, matches, kept = tree.place(listed, margin)
        per_read.append(NO_NODE if v is None else v)
        if v is None:
            continue
        row = t[tree.n if v == ABOVE else v]
        row[0] += 1
        row[1] += matches
        row[2] += kept
    return np.array(t, np.uint64).reshape(tree.n + 1, 3), np.array(per_read, np.uint32)


# ---- the command line's bytes -------------------------------------------------------------------------------------------
def names_of(nodes):
    """a name for most nodes, with blanks inside; every seventh has none"""
    return ["" if v % 7 == 3 else "taxon %d of %d-%d" % (v, lo, hi - 1) for v, (lo, hi) in enumerate(nodes)]


def taxonomy_file(nodes, names):
    """the bytes of a -T file: ids inclusive, a comment line first, blank lines and a tab here and there"""
    out = [b"# first_id last_id name\n"]
    for v, ((lo, hi), name) in enumerate(zip(nodes, names)):
        sep = b"\t" if v % 2 else b" "
        out.append(b"%d%s%d" % (lo, sep, hi - 1) + ((sep + name.encode()) if name else b"") + b"\n")
        if v % 5 == 0:
            out.append(b"\n")
    return b"".join(out)


def format_report(t, tree, names):
    """the bytes of `miekki -y`: a line per node whose subtree holds a read, in node order: node, depth, first id, last id,
    clade_reads, reads, best_matches, hits, name"""
    clade = [int(r[0]) for r in t[:tree.n]]
    for v in range(tree.n - 1, -1, -1):
        if tree.parent[v] is not None:
            clade[tree.parent[v]] += clade[v]
    return b"".join(b"%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (v, tree.depth[v], tree.nodes[v][0], tree.nodes[v][1] - 1, clade[v], int(t[v][0]),
                                                           int(t[v][1]), int(t[v][2]), names[v].encode())
                    for v in range(tree.n) if clade[v])


def format_reads(per_read):
    """the bytes of `miekki -Y`: ordinal, then the node, * above every node, - unassigned"""
    return b"".join(b"%d\t%s\n" % (i, b"-" if v == NO_NODE else b"*" if v == ABOVE else b"%d" % v) for i, v in enumerate(per_read))


def summary_line(t, n_queries, margin):
    t = np.asarray(t)
    return b"lca: %d queries, %d assigned, %d above every node, %d nodes with reads, margin %d" % (
        n_queries, int(t[:, 0].sum()), int(t[-1, 0]), int((t[:-1, 0] > 0).sum()), margin)


# ---- the grouped collection ---------------------------------------------------------------------------------------------
class Grouped:
    """fr.Collection(1101, fp_bits, 310_000)'s sequences permuted so that every planted group is a RUN of ids: species_a at
    254-258 (across the 256 step of the score walk), species_b at 510-513 (across the 512 step of the partial-count walk),
    the chain at 1022-1024 (the score tile's edge at 8 bits), the nested pair at 4 and 5 (inside one lane); every other
    genome keeps its order.  Reads cut as tally_ref.Sample cuts them -- 600 of 300-999 bases, every third from a planted
    genome, 20 unrelated ones -- plus eight whole genomes: a mixed set.  The oracle's rows of all of them, once."""

    RUNS = {"species_a": 254, "species_b": 510, "chain": 1022, "nested": 4}
    WHOLE = (254, 258, 510, 1022, 1024, 4, 5, 700)

    def __init__(self, G=1101, fp_bits=8, seed=310_000):
        self.c = c = fr.Collection(G, fp_bits, seed)
        at = {}
        for name, first in self.RUNS.items():
            for i, old in enumerate(getattr(c, name)):
                at[first + i] = old
        taken = set(at.values())
        rest = iter(g for g in range(G) if g not in taken)
        self.order = [at[j] if j in at else next(rest) for j in range(G)]   # new id j is the collection's genome order[j]
        assert sorted(self.order) == list(range(G))
        self.seqs = [c.seqs[g] for g in self.order]
        self.G, self.par = G, c.par
        self.planted = sorted(at)
        self.a = fr.Answer(c.par, self.seqs)
        self.o = self.a.o
        rng = np.random.default_rng(5)
        reads = []
        for i in range(600):
            g = int(rng.integers(0, G)) if i % 3 else int(rng.choice(self.planted))
            L = 300 + (i * 7) % 700
            off = int(rng.integers(0, max(1, len(self.seqs[g]) - L)))
            reads.append(self.seqs[g][off:off + L])
        reads += [synth.genome_bases(4_000_000 + i, 0, 800) for i in range(20)]
        self.reads = reads
        self.queries = reads + [self.seqs[g] for g in self.WHOLE]
        self.rows = self.o.query_sequences(self.queries)
        self.read_rows = self.rows[:len(reads)]
