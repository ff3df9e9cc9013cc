"""What does the base-quality cut cost in the sketch step?  (recorded, not gated: profiles/read_quality.txt)

The index of profiles/query_tally.txt -- synthetic strain genomes in families of 64 at -h 17 -- and reads of 150 bases cut from
genomes at random, ONE set of reads uploaded three ways and sketched (mk_qset_invalidate, mk_qset_active: sketch and Bloom
gate, no scan), one warm-up and --repeats timed sketches each (min / median / max of the device's own sketch_ms, and of a
host clock around the call, which ends in a device wait):
  (p)  mk_qset_upload                               the plain kernel -- run BEFORE and AFTER the others in the same job
  (q0) mk_qset_upload_reads at min_qual 0           the masked arm with nothing to cut
  (q)  mk_qset_upload_reads at min_qual 20          the masked arm, about one base in twenty below the threshold
and per route the sum of the active partitions.

--only-plain --lib PATH times route (p) alone with another build of the library (one without mk_qset_upload_reads will do):
the plain path of a build against its parent's, run alternately by a job script.

    python tools/read_quality_rate.py [--genomes 20000] [--reads 100000] [--out FILE] [--only-plain] [--lib PATH] [--tag NAME]
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
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--strains", type=int, default=64)
    ap.add_argument("--rate-ppm", type=int, default=3000)
    ap.add_argument("--h", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only-plain", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from miekki_amd import lib as L
    if args.lib:
        L._LIB_PATH = os.path.abspath(args.lib)
        have = C.CDLL(L._LIB_PATH)
        for name in [n for n in L.SIGNATURES if not hasattr(have, n)]:
            if not args.only_plain:
                raise SystemExit(f"{args.lib} has no {name}")
            del L.SIGNATURES[name]
    import miekki_amd
    import synth
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, N = args.genomes, args.reads
    ix = miekki_amd.Miekki(31, args.h, 8, 33, 200)
    ix.reserve(G)
    for g0 in range(0, G, 2048):
        ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
    L.check(lib.mk_sync(ix._h))
    rng = np.random.default_rng(9)
    distinct = min(N, 20_000)                                    # (the reads are cut on the host: the set repeats them)
    cut = [synth.strain_device(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 150)), 150)
           for _ in range(distinct)]
    reads = [cut[i % distinct] for i in range(N)]
    qual = np.full((distinct, 150), ord("I"), np.uint8)
    bad = rng.random((distinct, 150)) < 0.05
    qual[bad] = ord("#")
    quals = [qual[i % distinct].tobytes() for i in range(N)]
    say(f"{args.tag + ': ' if args.tag else ''}index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, "
        f"-k 31 -h {args.h}; {N} reads of 150 bases, {int(bad.sum()) * 100.0 / bad.size:.2f} % of the bases below 20; "
        f"{args.repeats} timed sketches after one warm-up: min / median / max")

    def route(tag, make):
        qs = C.c_void_p()
        make(qs)
        active = np.zeros(N, np.uint32)

        def one():
            L.check(lib.mk_qset_invalidate(ix._h, qs))
            L.check(lib.mk_qset_active(ix._h, qs, active.ctypes.data))

        one()                                                    # warm-up: code objects, buffers
        ts, sk = [], []
        for _ in range(args.repeats):
            ix.reset_stats()
            t = time.perf_counter()
            one()
            ts.append(time.perf_counter() - t)
            sk.append(ix.stats()["sketch_ms"])
        lib.mk_qset_free(ix._h, qs)
        say(f"  {tag}: sketch_ms {min(sk):6.3f} / {float(np.median(sk)):6.3f} / {max(sk):6.3f}   call wall "
            f"{min(ts) * 1e3:6.2f} / {float(np.median(ts)) * 1e3:6.2f} / {max(ts) * 1e3:6.2f} ms   active partitions {int(active.sum())}")

    p, l = L.seq_arrays(reads)
    x, _ = L.seq_arrays(quals)

    def plain(qs):
        L.check(lib.mk_qset_upload(ix._h, p, l, N, C.byref(qs)))

    def masked(min_qual):
        def make(qs):
            L.check(lib.mk_qset_upload_reads(ix._h, p, l, x, None, None, None, N, min_qual, C.byref(qs)))
        return make

    route("(p)  plain upload, first run     ", plain)
    if not args.only_plain:
        route("(q0) with qualities, min_qual 0  ", masked(0))
        route("(q)  with qualities, min_qual 20 ", masked(20))
        route("(p)  plain upload, second run    ", plain)
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
