"""What does placing every read in a taxonomy by lowest common ancestor cost beside the profile by clade, and beside the route
that was the only one before?  (recorded, not gated: profiles/read_lca.txt)

The inputs of profiles/clade_tally.txt -- 20,000 synthetic strain genomes in families of 64 at -h 17, 20,000 reads of 1 kb as
ONE uploaded set, invalidated before every pass so that a pass is complete (sketch, Bloom gate, scan, walk) -- and the
taxonomy root > families > a singleton leaf per genome.  Per pass mk_stats.filter_ms, which carries the walk's launches and
nothing else in the device routes; the scan is about a hundred times the walk, so the wall clock says little about it.  One
warm-up and --repeats timed passes (min / median / max of filter_ms):
  (c)  mk_qset_run_clade_tally, the families as clades   the yardstick: one walk with a map
  (a)  mk_qset_run_lca, margin 100                       one walk, the reduction, the climb
  (m)  mk_qset_run_lca, margin 10                        two walks for the reads that list more than one genome
  (n)  (m) with d_node, the nodes read back              4 bytes per read to the host
  (h)  mk_qset_run_list(MK_LIST_CANDIDATES) + the LCA    the only route before: every hit of every read to the host, then the
       of margin 10 on the host in numpy                 same rule there
and two read sets: reads cut from genomes drawn at random, and reads all cut from ONE genome.  The host route's counters and
nodes must equal the device's, and the identities of the definition are checked, before anything is reported.

    python tools/lca_rate.py [--genomes 20000] [--queries 20000] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HIT = np.dtype([("genome", "<u4"), ("matches", "<u4"), ("jaccard", "<f8"), ("intersection", "<f8")])
NO_NODE, ABOVE = 0xffffffff, 0xfffffffe


def host_lca(off, rec, leaf, parent, hi, n_nodes, margin):
    """the header's rule over the lists of all reads, in numpy: (counters [n_nodes + 1, 3], nodes [reads])"""
    off = np.asarray(off, np.int64)
    nq = len(off) - 1
    nodes = np.full(nq, NO_NODE, np.uint32)
    t = np.zeros((n_nodes + 1, 3), np.uint64)
    has = np.flatnonzero(np.diff(off) > 0)
    if not len(has) or not len(rec):
        return t, nodes
    g, x = rec["genome"].astype(np.int64), rec["intersection"]
    seg = np.repeat(np.arange(nq), np.diff(off))
    keep = leaf[g] != NO_NODE
    g, x, m, seg = g[keep], x[keep], rec["matches"][keep], seg[keep]
    start = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
    q = seg[start]
    best_x = np.maximum.reduceat(x, start)
    per = np.repeat(np.arange(len(start)), np.diff(np.r_[start, len(seg)]))
    ties = x == best_x[per]
    tie_g = np.full(len(start), -1)
    np.maximum.at(tie_g, per[ties], g[ties])                       # among equal intersections the largest id
    is_best = ties & (g == tie_g[per])
    best_m = np.zeros(len(start), np.uint64)
    best_m[per[is_best]] = m[is_best]
    kept = x * 100.0 >= best_x[per] * float(100 - margin)
    a = np.full(len(start), np.iinfo(np.int64).max)
    b = np.full(len(start), -1)
    np.minimum.at(a, per[kept], g[kept])
    np.maximum.at(b, per[kept], g[kept])
    n_kept = np.bincount(per[kept], minlength=len(start))
    v = leaf[a].astype(np.int64)
    while True:
        up = (v != NO_NODE) & (hi[np.minimum(v, n_nodes - 1)] <= b)
        if not up.any():
            break
        v[up] = parent[v[up]]
    slot = np.where(v == NO_NODE, n_nodes, v)
    t[:, 0] = np.bincount(slot, minlength=n_nodes + 1)
    t[:, 1] = np.bincount(slot, weights=best_m, minlength=n_nodes + 1).astype(np.uint64)
    t[:, 2] = np.bincount(slot, weights=n_kept, minlength=n_nodes + 1).astype(np.uint64)
    nodes[q] = np.where(v == NO_NODE, ABOVE, v).astype(np.uint32)
    return t, nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=20_000)
    ap.add_argument("--queries", type=int, default=20_000)
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--strains", type=int, default=64)
    ap.add_argument("--rate-ppm", type=int, default=3000)
    ap.add_argument("--h", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import miekki_amd
    import synth
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, NQ, thr = args.genomes, args.queries, 200
    mi = 0.5 * thr
    ix = miekki_amd.Miekki(31, args.h, 8, 33, thr)
    ix.reserve(G)
    for g0 in range(0, G, 2048):
        ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
    L.check(lib.mk_sync(ix._h))
    # root > families > singleton leaves, in preorder
    lo, hi = [0], [G]
    for f0 in range(0, G, args.strains):
        f1 = min(G, f0 + args.strains)
        lo.append(f0); hi.append(f1)
        lo += list(range(f0, f1)); hi += list(range(f0 + 1, f1 + 1))
    lo, hi = np.array(lo, np.uint32), np.array(hi, np.uint32)
    n_nodes = len(lo)
    n_slots = n_nodes + 1
    tax = C.c_void_p()
    L.check(lib.mk_taxonomy_create(ix._h, lo.ctypes.data, hi.ctypes.data, n_nodes, G, C.byref(tax)))
    parent = np.zeros(n_nodes, np.uint32)
    L.check(lib.mk_taxonomy_parents(tax, parent.ctypes.data))
    leaf = np.flatnonzero(hi - lo == 1).astype(np.uint32)           # (every genome has its singleton)
    family_node = np.flatnonzero((hi - lo > 1) & (np.arange(n_nodes) > 0))
    assert len(leaf) == G and (lo[leaf] == np.arange(G)).all()
    fam_of = (np.arange(G) // args.strains).astype(np.uint32)
    cmap = C.c_void_p()
    L.check(lib.mk_clade_map_create(ix._h, fam_of.ctypes.data, G, C.byref(cmap)))
    n_clades = int(fam_of.max()) + 1
    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; "
        f"{NQ} reads of 1 kb, thresholds (10, {mi}); taxonomy: a root, {n_clades} families, {G} leaves; "
        f"{args.repeats} timed passes after one warm-up: filter_ms min / median / max")
    d_lt, d_ct, d_node = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, 24 * n_slots, C.byref(d_lt)))
    L.check(lib.mk_dev_alloc(ix._h, 40 * n_clades, C.byref(d_ct)))
    L.check(lib.mk_dev_alloc(ix._h, 4 * NQ, C.byref(d_node)))

    def case(name, reads):
        ptrs, lens = L.seq_arrays(reads)
        qs = C.c_void_p()
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))

        def one_pass(which):
            """(filter_ms, scan_ms, wall, counters, nodes or None, bytes to the host)"""
            ix.reset_stats()
            nodes = None
            t0 = time.perf_counter()
            L.check(lib.mk_qset_invalidate(ix._h, qs))
            if which == "c":
                out = np.zeros((n_clades, 5), np.uint64)
                L.check(lib.mk_clade_tally_reset(ix._h, d_ct, n_clades))
                L.check(lib.mk_qset_run_clade_tally(ix._h, qs, 10, mi, cmap, d_ct, n_clades, None, 0))
                L.check(lib.mk_clade_tally_read(ix._h, d_ct, n_clades, out.ctypes.data))
                nbytes = out.nbytes
            elif which == "h":
                hl = C.c_void_p()
                L.check(lib.mk_qset_run_list(ix._h, qs, L.LIST_CANDIDATES, 10, mi, C.byref(hl)))
                off = np.ctypeslib.as_array(lib.mk_hitlist_offsets(hl), (NQ + 1,)).copy()
                rec = np.zeros(int(off[NQ]), HIT)
                if len(rec):
                    C.memmove(rec.ctypes.data, lib.mk_hitlist_hits(hl), rec.nbytes)
                lib.mk_hitlist_free(hl)
                out, nodes = host_lca(off, rec, leaf, parent, hi, n_nodes, 10)
                nbytes = rec.nbytes + 20 * NQ + 16                     # (as tools/tally_rate.py counts a list call)
            else:
                margin, want_nodes = {"a": (100, False), "m": (10, False), "n": (10, True)}[which]
                out = np.zeros((n_slots, 3), np.uint64)
                L.check(lib.mk_lca_tally_reset(ix._h, d_lt, n_slots))
                L.check(lib.mk_qset_run_lca(ix._h, qs, 10, mi, margin, tax, d_lt, n_slots, d_node if want_nodes else None))
                if want_nodes:
                    nodes = np.zeros(NQ, np.uint32)
                    L.check(lib.mk_dev_download(ix._h, nodes.ctypes.data, d_node, nodes.nbytes))
                L.check(lib.mk_lca_tally_read(ix._h, d_lt, n_slots, out.ctypes.data))
                nbytes = out.nbytes + (nodes.nbytes if want_nodes else 0)
            wall = time.perf_counter() - t0
            s = ix.stats()
            return s["filter_ms"], s["scan_ms"], wall, out, nodes, nbytes

        def timed(which):
            one_pass(which)                                              # warm-up: code objects, buffers
            got = [one_pass(which) for _ in range(args.repeats)]
            f = sorted(g[0] for g in got)
            return (f[0], float(np.median(f)), f[-1]), float(np.median([g[1] for g in got])), float(np.median([g[2] for g in got])), got[-1][3:]

        rows = [(f"(c) clade pass, families of {args.strains:<3}        ", timed("c")),
                ("(a) lca pass, margin 100               ", timed("a")),
                ("(m) lca pass, margin 10                ", timed("m")),
                ("(n) (m) with the nodes read back       ", timed("n")),
                ("(h) all hits to the host + numpy LCA   ", timed("h"))]
        clade, at100, at10, with_nodes, host = (r[1][3][0] for r in rows)
        ok = (np.array_equal(at10, with_nodes) and np.array_equal(host, at10) and np.array_equal(rows[4][1][3][1], rows[3][1][3][1])
              and int(at100[:, 0].sum()) == int(at10[:, 0].sum()) == int(clade[:, 2].sum())       # all slots: the assigned reads
              and at100[n_nodes, 0] == 0 and at10[n_nodes, 0] == 0                                 # one root: nothing above it
              and int(at100[family_node, 0].sum() + at100[leaf, 0].sum()) == int(clade[:, 1].sum()))   # below the root: one family only
        if not ok:
            raise SystemExit(f"{name}: the routes disagree or the counters break an identity of the definition")

        def levels(t):
            return f"root {int(t[0, 0])}, families {int(t[family_node, 0].sum())}, leaves {int(t[leaf, 0].sum())}"
        say(f"{name}: {int(at100[:, 0].sum())} reads assigned; margin 100: {levels(at100)}, {int(at100[:, 2].sum())} hits; "
            f"margin 10: {levels(at10)}, {int(at10[:, 2].sum())} hits; the host route agrees, identities hold")
        for tag, (f, scan, wall, (_, _, nbytes)) in rows:
            say(f"  {tag}: filter_ms {f[0]:6.2f} / {f[1]:6.2f} / {f[2]:6.2f}   scan_ms {scan:6.1f}   wall {wall * 1e3:6.1f} ms   to the host: {nbytes} bytes")
        c_med, a_med, m_med = (r[1][0][1] for r in rows[:3])
        say(f"  (a) / (c): {a_med / c_med:.2f}   (m) / (c): {m_med / c_med:.2f}   wall (h) / (n): {rows[4][1][2] / rows[3][1][2]:.2f}")
        lib.mk_qset_free(ix._h, qs)

    rng = np.random.default_rng(8)
    spread = []
    for _ in range(NQ):
        g = int(rng.integers(0, G))
        spread.append(synth.strain_device(g, args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000)), 1000))
    case("case 1, reads from genomes at random", spread)
    g = G // 2 + 7
    one = [synth.strain_device(g, args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000)), 1000) for _ in range(NQ)]
    case(f"case 2, reads from genome {g} alone", one)
    lib.mk_taxonomy_free(ix._h, tax)
    lib.mk_clade_map_free(ix._h, cmap)
    for p in (d_lt, d_ct, d_node):
        lib.mk_dev_free(ix._h, p)
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
