"""What does the profile of a read set BY CLADE cost beside the profile by genome?  (recorded, not gated:
profiles/clade_tally.txt)

The inputs of profiles/query_tally.txt -- 20,000 synthetic strain genomes in families of 64 at -h 17, 20,000 reads of 1 kb as
ONE uploaded set, invalidated before every pass so that a pass is complete (sketch, Bloom gate, scan, walk) -- and per pass
mk_stats.filter_ms, which carries the walk's launches and nothing else here; the scan is about a hundred times the walk, so
the wall clock says little.  One warm-up and --repeats timed passes (min / median / max of filter_ms):
  (t) mk_qset_run_tally                                  the unchanged tally_kernel: the yardstick
  (s) mk_qset_run_clade_tally, clade[j] = j              singleton clades: the same adds, plus the map and the ballot
  (f) mk_qset_run_clade_tally, clade[j] = j / strains    the families: `listed` once per read and family
  (o) mk_qset_run_clade_tally, clade[j] = 0              one clade of all genomes: every add lands on one row of counters
  (b) (f) with d_tally given                             both sinks on each chunk of one scan
  (2) (t), then (f)                                      the same two results from two passes
and two read sets: reads cut from genomes drawn at random, and reads all cut from ONE genome (the worst case for the
atomics of the plain tally).  The identities of the definition are checked on the counters before anything is reported.

    python tools/clade_rate.py [--genomes 20000] [--queries 20000] [--out FILE]
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
    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; "
        f"{NQ} reads of 1 kb, thresholds (10, {mi}); {args.repeats} timed passes after one warm-up: filter_ms min / median / max")
    d_tally, d_ct = C.c_void_p(), C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, 32 * G, C.byref(d_tally)))
    L.check(lib.mk_dev_alloc(ix._h, 40 * G, C.byref(d_ct)))
    maps = {}
    for tag, clade in (("s", np.arange(G, dtype=np.uint32)), ("f", (np.arange(G) // args.strains).astype(np.uint32)), ("o", np.zeros(G, np.uint32))):
        m = C.c_void_p()
        L.check(lib.mk_clade_map_create(ix._h, clade.ctypes.data, G, C.byref(m)))
        maps[tag] = (m, int(clade.max()) + 1, clade)

    def case(name, reads):
        ptrs, lens = L.seq_arrays(reads)
        qs = C.c_void_p()
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))

        def passes(*which):
            """the passes named, each behind an invalidate: (filter_ms of all, scan_ms of all, wall, tally, clade counters)"""
            tally, ct = np.zeros((G, 4), np.uint64), None
            L.check(lib.mk_tally_reset(ix._h, d_tally, G))
            ix.reset_stats()
            t = time.perf_counter()
            for w in which:
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                if w == "t":
                    L.check(lib.mk_qset_run_tally(ix._h, qs, 10, mi, d_tally, G))
                else:
                    m, n, _ = maps[w[0]]
                    L.check(lib.mk_clade_tally_reset(ix._h, d_ct, n))
                    L.check(lib.mk_qset_run_clade_tally(ix._h, qs, 10, mi, m, d_ct, n, d_tally if w.endswith("+t") else None, G))
                    ct = np.zeros((n, 5), np.uint64)
            if ct is not None:
                L.check(lib.mk_clade_tally_read(ix._h, d_ct, len(ct), ct.ctypes.data))
            L.check(lib.mk_tally_read(ix._h, d_tally, G, tally.ctypes.data))
            wall = time.perf_counter() - t
            s = ix.stats()
            return s["filter_ms"], s["scan_ms"], wall, tally, ct

        def timed(*which):
            passes(*which)                                           # warm-up: code objects, buffers
            got = [passes(*which) for _ in range(args.repeats)]
            f = sorted(g[0] for g in got)
            return (f[0], float(np.median(f)), f[-1]), float(np.median([g[1] for g in got])), float(np.median([g[2] for g in got])), got[-1][3], got[-1][4]

        rows = [("(t) tally_kernel, per genome        ", timed("t")),
                ("(s) clade pass, singleton clades    ", timed("s")),
                (f"(f) clade pass, families of {args.strains:<3}    ", timed("f")),
                ("(o) clade pass, one clade of all    ", timed("o")),
                ("(b) (f) with d_tally, one scan      ", timed("f+t")),
                ("(2) (t) then (f), two scans         ", timed("t", "f"))]
        tally = rows[0][1][3]
        single, fam, one, both, two = (r[1][4] for r in rows[1:])
        fam_of = maps["f"][2]
        ok = (np.array_equal(single[:, :4], tally) and np.array_equal(single[:, 4], tally[:, 0])
              and one[0, 0] == one[0, 1] == one[0, 2] == tally[:, 2].sum() and one[0, 4] == tally[:, 0].sum()
              and np.array_equal(fam[:, 4], np.bincount(fam_of, weights=tally[:, 0], minlength=len(fam)).astype(np.uint64))
              and np.array_equal(fam[:, 2], np.bincount(fam_of, weights=tally[:, 2], minlength=len(fam)).astype(np.uint64))
              and np.array_equal(fam[:, 3], np.bincount(fam_of, weights=tally[:, 3], minlength=len(fam)).astype(np.uint64))
              and np.array_equal(both, fam) and np.array_equal(two, fam)
              and np.array_equal(rows[4][1][3], tally) and np.array_equal(rows[5][1][3], tally))
        if not ok:
            raise SystemExit(f"{name}: the counters break an identity of the definition")
        say(f"{name}: {int(tally[:, 0].sum())} (read, genome) pairs listed, {int(fam[:, 0].sum())} (read, family) pairs, "
            f"{int(fam[:, 1].sum())} of {int(fam[:, 2].sum())} assigned reads list one family only ({int(tally[:, 1].sum())} one genome only); identities hold")
        for tag, (f, scan, wall, _, _) in rows:
            say(f"  {tag}: filter_ms {f[0]:6.2f} / {f[1]:6.2f} / {f[2]:6.2f}   scan_ms {scan:6.1f}   wall {wall * 1e3:6.1f} ms")
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
    for m, _, _ in maps.values():
        lib.mk_clade_map_free(ix._h, m)
    lib.mk_dev_free(ix._h, d_ct)
    lib.mk_dev_free(ix._h, d_tally)
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
