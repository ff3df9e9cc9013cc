"""What does the node pass of mk_taxonomy_cover cost beside the passes it resembles?  (recorded, not gated: profiles/taxon_cover.txt)

The index of profiles/sample_cover.txt -- 20,000 synthetic strain genomes in families of 64 at -k 31 -h 17 -- and 20,000 reads of
1 kb cut from genomes drawn at random, marked into a cover table once; the taxonomy root > 313 families > 20,000 leaves.  Then, on
that table, from the same run, one warm-up and --repeats timed calls each (min / median / max of the device's own event times,
mk_stats filter_ms; the host clock around the call beside it), at one byte and at two:
  count      mk_cover_count                         one streaming read of the matrix: the yardstick of the narrow path
  assign     mk_cover_assign, the natural order     the win pass: the loop the wide path has
  full       mk_taxonomy_cover, all three levels    the node pass over root and families, and the count pass for the leaves
  nodes      ... root and families only             the node pass alone: 2 x the matrix's genome bytes
  root       ... the root only                      by the default width, and with every node forced wide / narrow
  families   ... the 313 families only              likewise (MIEKKI_TAXCOVER_WIDE=2 / above G)
with the bytes each reads (sum over the nodes of width >= 2 of width x P x W) and the GB/s.  The identities are checked on the
way: the root's covered is mk_cover_winners' claimed, the leaves are sketch_size and mk_cover_count's covered, every path gives
the same counts.

    python tools/taxon_cover_rate.py [--genomes 20000] [--out FILE]
"""
import argparse
import ctypes as C
import multiprocessing
import os
import sys
import time

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
    G, NQ, P = args.genomes, args.queries, 1 << args.h
    # the reads first, in worker processes that never see the device
    rng = np.random.default_rng(8)
    jobs = [(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(NQ)]
    with multiprocessing.get_context("fork").Pool(args.workers) as pool:
        reads = pool.map(cut, jobs, chunksize=2000)
    import miekki_amd
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def mmm(a):
        return f"{np.min(a):8.3f} / {np.median(a):8.3f} / {np.max(a):8.3f}"

    root = [(0, G)]
    families = [(g, min(g + args.strains, G)) for g in range(0, G, args.strains)]
    leaves = [(g, g + 1) for g in range(G)]
    full = sorted(root + families + leaves, key=lambda n: (n[0], -n[1]))

    def one_width(bits):
        W = bits // 8
        ix = miekki_amd.Miekki(31, args.h, bits, 33, 200)
        ix.reserve(G)
        for g0 in range(0, G, 2048):
            ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
        L.check(lib.mk_sync(ix._h))
        d_seen = C.c_void_p()
        L.check(lib.mk_dev_alloc(ix._h, lib.mk_cover_bytes(ix._h), C.byref(d_seen)))
        ptrs, lens = L.seq_arrays(reads)
        qs = C.c_void_p()
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))
        L.check(lib.mk_cover_reset(ix._h, d_seen))
        L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen))
        L.check(lib.mk_sync(ix._h))
        lib.mk_qset_free(ix._h, qs)
        say(f"{bits}-bit fingerprints: matrix {P * ((G * W + 1023) // 1024 * 1024)} bytes ({P * G * W} of genomes), table {lib.mk_cover_bytes(ix._h)} bytes")

        def timed(fn, env=None):
            for k, v in (env or {}).items():
                os.environ[k] = v
            try:
                fn()                                                 # warm-up: code objects, buffers
                ts, dev = [], []
                for _ in range(args.repeats):
                    ix.reset_stats()
                    t = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t)
                    dev.append(ix.stats()["filter_ms"])
            finally:
                for k in env or {}:
                    del os.environ[k]
            return np.array(ts) * 1e3, np.array(dev)

        cov, won = np.zeros(G, np.uint32), np.zeros(G, np.uint32)
        cells, claimed = C.c_uint64(0), C.c_uint64(0)
        L.check(lib.mk_cover_winners(ix._h, d_seen, cov.ctypes.data, won.ctypes.data, C.byref(cells), C.byref(claimed)))
        order = np.arange(G, dtype=np.uint32)
        t, d = timed(lambda: L.check(lib.mk_cover_count(ix._h, d_seen, cov.ctypes.data, C.byref(cells))))
        count_ms = float(np.median(d))
        say(f"  count                      : wall {mmm(t)}   device {mmm(d)}   {P * G * W / count_ms / 1e6:7.0f} GB/s")
        t, d = timed(lambda: L.check(lib.mk_cover_assign(ix._h, d_seen, order.ctypes.data, won.ctypes.data, None)))
        assign_ms = float(np.median(d))
        say(f"  assign                     : wall {mmm(t)}   device {mmm(d)}   {P * G * W / assign_ms / 1e6:7.0f} GB/s")

        def node_pass(label, nodes, env=None, against=None):
            lo = np.array([n[0] for n in nodes], np.uint32)
            hi = np.array([n[1] for n in nodes], np.uint32)
            tax = C.c_void_p()
            L.check(lib.mk_taxonomy_create(ix._h, lo.ctypes.data, hi.ctypes.data, len(nodes), G, C.byref(tax)))
            nc, n_cells = np.zeros((len(nodes), 2), np.uint64), C.c_uint64(0)
            t, d = timed(lambda: L.check(lib.mk_taxonomy_cover(ix._h, tax, d_seen, nc.ctypes.data, C.byref(n_cells))), env)
            lib.mk_taxonomy_free(ix._h, tax)
            nbytes = sum((b - a) * P * W for a, b in nodes if b - a >= 2)
            ms = float(np.median(d))
            vs = "" if against is None else f"   = {ms / against[1]:.2f} x {against[0]}"
            say(f"  {label:<27}: wall {mmm(t)}   device {mmm(d)}   {nbytes} bytes, {nbytes / ms / 1e6:7.0f} GB/s{vs}")
            assert n_cells.value == cells.value
            return nc

        nc = node_pass("full, three levels", full)
        width = np.array([b - a for a, b in full])
        assert int(nc[0, 1]) == claimed.value                                 # the root is the winners' claimed
        assert (nc[width == 1, 0] == ix.sketch_size).all() and (nc[width == 1, 1] == cov).all()
        assert (nc[:, 1] <= nc[:, 0]).all()
        fam = nc[width == args.strains]
        say(f"    cells {cells.value}; root: held {int(nc[0, 0])}, covered {int(nc[0, 1])} (claimed {claimed.value}); sum of the leaves' held "
            f"{int(ix.sketch_size.sum())}, covered {int(cov.sum())}; families: median held {int(np.median(fam[:, 0]))}, median covered / held "
            f"{float(np.median(fam[:, 1] / np.maximum(fam[:, 0], 1))):.4f}, noise floor {cells.value / (P << bits):.4f}")
        both = node_pass("nodes: root and families", root + families)
        at = {n: i for i, n in enumerate(full)}
        assert (both == nc[[at[n] for n in root + families]]).all()         # the same counts beside the leaves and without them
        wide, narrow = {"MIEKKI_TAXCOVER_WIDE": "2"}, {"MIEKKI_TAXCOVER_WIDE": str(G + 1)}
        r0 = node_pass("root", root, None, ("assign", assign_ms))
        for label, env in (("root, forced wide", wide), ("root, forced narrow", narrow)):
            assert (node_pass(label, root, env, ("assign", assign_ms)) == r0).all()
        f0 = node_pass("families", families, None, ("count", count_ms))
        assert (node_pass("families, forced wide", families, wide, ("assign", assign_ms)) == f0).all()
        assert (node_pass("families, forced narrow", families, narrow, ("count", count_ms)) == f0).all()
        lib.mk_dev_free(ix._h, d_seen)
        ix.close()

    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; {NQ} reads of 1 kb from "
        f"genomes at random; taxonomy: root > {len(families)} families > {G} leaves; {args.repeats} timed calls after one warm-up: min / median / max (ms)")
    for bits in (8, 16):
        one_width(bits)
    say("(tools/taxon_cover_rate.py; device: mk_stats filter_ms; wall: host clock around calls that end in a device wait; one MI355X.)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
