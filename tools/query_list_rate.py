"""What does "every genome above the thresholds" cost?  (recorded, not gated: profiles/r8_query_list.txt)

20,000 synthetic strain genomes in families of 64 (mk_index_append_synthetic_strains) at -h 17, 20,000 queries of 1 kb
cut from them, and three routes over the same queries, each timed by a host clock around the C call (every call ends
in a device wait), one warm-up and --repeats timed passes:
  (a) mk_query(nresults = 10)                 the reference's ten
  (b) mk_query_list(MK_ALL_RESULTS)           every genome above the thresholds, ordered on the device
  (c) mk_query(nresults = index_size)         the only route to (b)'s answer before mk_query_list: a launch, a copy and
                                              a wait per query -- on a 1/20 sample, scaled, when the whole set would take
                                              more than a minute
plus the passing genomes per query (mean, p99, max) and the bytes of hits (b) returns.

    python tools/query_list_rate.py [--genomes 20000] [--queries 20000] [--out FILE]
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
    ap.add_argument("--repeats", type=int, default=3)
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
    ix = miekki_amd.Miekki(31, args.h, 8, 33, thr)
    ix.reserve(G)
    t0 = time.perf_counter()
    for g0 in range(0, G, 2048):
        ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
    L.check(lib.mk_sync(ix._h))
    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}, "
        f"built in {time.perf_counter() - t0:.1f} s")
    rng = np.random.default_rng(8)
    qs = []
    for _ in range(NQ):
        g = int(rng.integers(0, G))
        qs.append(synth.strain_device(g, args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000)), 1000))
    ptrs, lens = L.seq_arrays(qs)
    mi = 0.5 * thr

    def timed(fn):
        fn()                                                     # warm-up: code objects, buffers
        ts = []
        for _ in range(args.repeats):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return min(ts), float(np.median(ts))

    def stats_ms():
        s = ix.stats()
        return s["sketch_ms"], s["scan_ms"], s["filter_ms"]

    hits10 = (L.Hit * (NQ * 10))()
    nh = np.zeros(NQ, np.uint32)

    def run_a():
        ix.reset_stats()
        L.check(lib.mk_query(ix._h, ptrs, lens, NQ, 10, 10, mi, hits10, nh.ctypes.data, None))
    a_min, a_med = timed(run_a)
    a_dev = stats_ms()
    say(f"(a) mk_query(nresults=10), {NQ} queries:            min {a_min:.3f} s  median {a_med:.3f} s   "
        f"device ms: sketch {a_dev[0]:.1f} scan {a_dev[1]:.1f} filter {a_dev[2]:.1f}")

    got = {}

    def run_b():
        ix.reset_stats()
        hl = C.c_void_p()
        L.check(lib.mk_query_list(ix._h, ptrs, lens, NQ, L.ALL_RESULTS, 10, mi, C.byref(hl), None))
        got["off"] = np.ctypeslib.as_array(lib.mk_hitlist_offsets(hl), (NQ + 1,)).copy()
        lib.mk_hitlist_free(hl)
    b_min, b_med = timed(run_b)
    b_dev = stats_ms()
    per = np.diff(got["off"])
    say(f"(b) mk_query_list(MK_ALL_RESULTS), {NQ} queries:    min {b_min:.3f} s  median {b_med:.3f} s   "
        f"device ms: sketch {b_dev[0]:.1f} scan {b_dev[1]:.1f} filter {b_dev[2]:.1f}")
    say(f"    passing genomes per query: mean {per.mean():.1f}  p99 {np.percentile(per, 99):.0f}  max {per.max()}; "
        f"hits returned: {int(got['off'][-1]) * 24} bytes")

    ns = max(1, NQ // 20)
    hitsG = (L.Hit * (ns * G))()
    nhs = np.zeros(ns, np.uint32)

    def run_c(q0):
        sp = (C.c_char_p * ns)(*qs[q0:q0 + ns])
        sl = (C.c_uint64 * ns)(*[len(s) for s in qs[q0:q0 + ns]])
        L.check(lib.mk_query(ix._h, sp, sl, ns, G, 10, mi, hitsG, nhs.ctypes.data, None))
    c_min, c_med = timed(lambda: run_c(0))
    if c_min * (NQ / ns) > 60.0 or ns == NQ:
        say(f"(c) mk_query(nresults={G}), {ns} of the queries:   min {c_min:.3f} s  median {c_med:.3f} s   "
            f"-> SCALED x{NQ / ns:.0f} to {NQ} queries: {c_min * NQ / ns:.1f} s")
        c_all = c_min * NQ / ns
    else:
        t = time.perf_counter()
        for q0 in range(0, NQ - ns + 1, ns):                     # (the route is per query: slices cost what the whole set costs)
            run_c(q0)
        c_all = time.perf_counter() - t
        say(f"(c) mk_query(nresults={G}), {NQ} queries in slices of {ns}: {c_all:.3f} s (one pass; sample of {ns}: min {c_min:.3f} s)")
    say(f"(b) / (a) = {b_min / a_min:.2f}   (c) / (b) = {c_all / b_min:.1f}")
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
