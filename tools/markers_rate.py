"""What does the marker pass cost beside the win pass it is shaped as?  (recorded, not gated: profiles/taxon_markers.txt)

The index of profiles/sample_cover.txt -- 20,000 synthetic strain genomes in families of 64 at -k 31 -h 17 -- and 20,000 reads
of 1 kb cut from genomes drawn at random, marked into a cover table once; then, on that table, from the same run, one warm-up
and --repeats timed passes each (min / median / max of the device's own event times on the library's stream, mk_stats
filter_ms), at one byte and at two:
  markers   mk_taxonomy_markers over root / 313 families / 20,000 leaves
  win       mk_cover_assign                          the yardstick: the same loop, one LDS atomic and a rank lookup where the
                                                     marker pass does two atomics and a climb
  count     mk_cover_count                           one count pass
  -U        mk_taxonomy_cover over the same taxonomy the node pass
and the marker pass with MIEKKI_MARK_FILTER=0, at two bytes with each MIEKKI_MARK_VALUES and with MIEKKI_MARK_TOUCHED=0.
The contention case: the same index under a forest of 20,000 singleton roots -- every shared cell goes to the ONE slot above
every node -- beside a single root over the same leaves, where the same cells go to the root.
And what the numbers say about the index: specific of the families and of the leaves.

    python tools/markers_rate.py [--genomes 20000] [--out FILE]
"""
import argparse
import ctypes as C
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cut(job):
    import synth
    g, strains, ppm, off = job
    return synth.strain_device(g, strains, ppm, off, 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=20_000)
    ap.add_argument("--queries", type=int, default=20_000)
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--strains", type=int, default=64)
    ap.add_argument("--rate-ppm", type=int, default=3000)
    ap.add_argument("--h", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G, NQ = args.genomes, args.queries
    rng = np.random.default_rng(8)
    jobs = [(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(NQ)]
    with multiprocessing.get_context("fork").Pool(args.workers) as pool:      # (worker processes that never see the device)
        reads = pool.map(cut, jobs, chunksize=2000)
    import miekki_amd
    import winners_ref as wr
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    families = [(g, min(G, g + args.strains)) for g in range(0, G, args.strains)]
    leaves = [(g, g + 1) for g in range(G)]
    levels = sorted([(0, G)] + families + leaves, key=lambda n: (n[0], -n[1]))
    rooted = [(0, G)] + leaves
    n_fam = len(families)

    def mmm(a):
        return f"{np.min(a):9.3f} / {np.median(a):9.3f} / {np.max(a):9.3f}"

    def timed(ix, fn, env=None, repeats=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            fn()                                                 # warm-up: code objects, buffers
            dev = []
            for _ in range(repeats or args.repeats):
                ix.reset_stats()
                fn()
                dev.append(ix.stats()["filter_ms"])
        finally:
            for k in env or {}:
                del os.environ[k]
        return np.array(dev)

    def taxonomy(ix, nodes):
        lo = np.array([n[0] for n in nodes], np.uint32)
        hi = np.array([n[1] for n in nodes], np.uint32)
        t = C.c_void_p()
        L.check(lib.mk_taxonomy_create(ix._h, lo.ctypes.data, hi.ctypes.data, len(nodes), G, C.byref(t)))
        return t

    def one_width(bits, switches):
        ix = miekki_amd.Miekki(31, args.h, bits, 33, 200)
        ix.reserve(G)
        for g0 in range(0, G, 2048):
            ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
        L.check(lib.mk_sync(ix._h))
        matrix = (1 << args.h) * ((G * (bits // 8) + 1023) // 1024 * 1024)
        say(f"{bits}-bit fingerprints: matrix {matrix} bytes, table {lib.mk_cover_bytes(ix._h)} bytes")
        d_seen = C.c_void_p()
        L.check(lib.mk_dev_alloc(ix._h, lib.mk_cover_bytes(ix._h), C.byref(d_seen)))
        ptrs, lens = L.seq_arrays(reads)
        qs = C.c_void_p()
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))
        L.check(lib.mk_cover_reset(ix._h, d_seen))
        L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen))
        L.check(lib.mk_sync(ix._h))
        lib.mk_qset_free(ix._h, qs)
        cov, won = np.zeros(G, np.uint32), np.zeros(G, np.uint32)
        cells, claimed = C.c_uint64(0), C.c_uint64(0)
        L.check(lib.mk_cover_winners(ix._h, d_seen, cov.ctypes.data, won.ctypes.data, C.byref(cells), C.byref(claimed)))
        order = wr.order(cov, ix.sketch_size).astype(np.uint32)
        t_levels, t_rooted, t_forest = taxonomy(ix, levels), taxonomy(ix, rooted), taxonomy(ix, leaves)
        nm = np.zeros((len(levels) + 1, 2), np.uint64)
        nm2 = np.zeros((len(rooted) + 1, 2), np.uint64)
        nc = np.zeros((len(levels), 2), np.uint64)

        def markers(t=t_levels, out=nm):
            L.check(lib.mk_taxonomy_markers(ix._h, t, d_seen, out.ctypes.data, len(out), None))

        d_mark = timed(ix, markers)
        want = nm.copy()
        assert int(nm[:, 1].sum()) == claimed.value
        d_win = timed(ix, lambda: L.check(lib.mk_cover_assign(ix._h, d_seen, order.ctypes.data, won.ctypes.data, None)))
        d_count = timed(ix, lambda: L.check(lib.mk_cover_count(ix._h, d_seen, cov.ctypes.data, None)))
        d_node = timed(ix, lambda: L.check(lib.mk_taxonomy_cover(ix._h, t_levels, d_seen, nc.ctypes.data, None)))
        m = np.median(d_mark)
        say(f"  markers, root / {n_fam} families / {G} leaves : {mmm(d_mark)} ms   = {m / np.median(d_win):.2f} x the win pass, "
            f"{m / np.median(d_count):.2f} x a count pass, {m / np.median(d_node):.2f} x the -U node pass; {matrix / m / 1e6:.0f} GB/s over the matrix bytes")
        say(f"  win pass (mk_cover_assign)                   : {mmm(d_win)} ms")
        say(f"  count pass (mk_cover_count)                  : {mmm(d_count)} ms")
        say(f"  -U node pass (mk_taxonomy_cover)             : {mmm(d_node)} ms")
        for label, env, repeats in switches:
            d = timed(ix, markers, env, repeats)
            assert (nm == want).all()
            say(f"  markers, {label:<36}: {mmm(d)} ms   = {np.median(d) / m:.2f} x the default")
        d_rooted = timed(ix, lambda: markers(t_rooted, nm2))
        root_cells = nm2[0].copy()
        d_forest = timed(ix, lambda: markers(t_forest, nm2[1:]))
        assert (nm2[-1] == root_cells).all()
        spread = max(np.max(d_rooted) - np.min(d_rooted), np.max(d_forest) - np.min(d_forest))
        say(f"  contention: one root over {G} leaves           : {mmm(d_rooted)} ms   ({int(root_cells[0])} cells go to the root)")
        say(f"  contention: a forest of {G} singleton roots    : {mmm(d_forest)} ms   (the same cells go to the slot above every node); "
            f"medians differ by {abs(np.median(d_forest) - np.median(d_rooted)):.3f} ms, the repeats spread over {spread:.3f} ms")
        fam = [i for i, n in enumerate(levels) if 1 < n[1] - n[0] < G]
        leaf = [i for i, n in enumerate(levels) if n[1] - n[0] == 1]
        ss = ix.sketch_size.astype(np.float64)
        say(f"  specific: root {int(want[0, 0])}, above {int(want[-1, 0])}; families: sum {int(want[fam, 0].sum())}, median {int(np.median(want[fam, 0]))}, "
            f"min {int(want[fam, 0].min())}; leaves: sum {int(want[leaf, 0].sum())}, median {int(np.median(want[leaf, 0]))}, "
            f"leaves with none {int((want[leaf, 0] == 0).sum())}, median specific / sketch_size {float(np.median(want[leaf, 0] / np.maximum(ss, 1))):.4f}")
        say(f"  covered : root {int(want[0, 1])}; families: sum {int(want[fam, 1].sum())}, with a covered cell {int((want[fam, 1] > 0).sum())}; "
            f"leaves: sum {int(want[leaf, 1].sum())}, with a covered cell {int((want[leaf, 1] > 0).sum())}; table cells {cells.value}, claimed {claimed.value}")
        for t in (t_levels, t_rooted, t_forest):
            lib.mk_taxonomy_free(ix._h, t)
        lib.mk_dev_free(ix._h, d_seen)
        ix.close()

    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; {NQ} reads of 1 kb from "
        f"genomes at random; {args.repeats} timed passes after one warm-up: min / median / max of mk_stats filter_ms (device events)")
    one_width(8, [("MIEKKI_MARK_FILTER=0", {"MIEKKI_MARK_FILTER": "0"}, None)])
    one_width(16, [("MIEKKI_MARK_FILTER=0", {"MIEKKI_MARK_FILTER": "0"}, None),
                   ("MIEKKI_MARK_TOUCHED=0", {"MIEKKI_MARK_TOUCHED": "0"}, None)] +
                  [(f"MIEKKI_MARK_VALUES={v}", {"MIEKKI_MARK_VALUES": str(v)}, 2 if v < 2048 else None) for v in (256, 512, 1024, 2048, 4096, 8192, 16384)])
    say("(tools/markers_rate.py; one MI355X.)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
