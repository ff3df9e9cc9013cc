"""What does a read pair cost as ONE query, against its two mates as two reads?  (recorded, not gated:
profiles/read_pairs.txt)

The index of profiles/query_tally.txt -- 20,000 synthetic strain genomes in families of 64 at -h 17 -- and 20,000 fragments of
400 bases cut from genomes at random.  Three routes through a complete profile pass (mk_qset_invalidate, mk_tally_reset,
mk_qset_run_tally, mk_tally_read: sketch, Bloom gate, scan, walk), each timed by a host clock around calls that end in a device
wait, one warm-up and --repeats timed passes (min / median / max), with the device's own sketch_ms beside it:
  (a) 20,000 pairs of 2 x 150 bases, mate 2 reverse-complemented      mk_qset_upload_pairs: the paired sketch kernel
  (b) the same 40,000 mates as single reads                            mk_qset_upload: the only route before pairs
  (c) 20,000 single reads of 300 bases (a fragment's first 300)        about as many k-mers per query as (a), unpaired kernel
and per route the reads assigned (the sum of `best`) and the sum of `unique`.

--only-c --lib PATH times route (c) alone with another build of the library (one without mk_qset_upload_pairs will do): the
unpaired path of a build against its parent's, run alternately by a job script.

    python tools/pairs_rate.py [--genomes 20000] [--fragments 20000] [--out FILE] [--only-c] [--lib PATH] [--tag NAME]
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

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=20_000)
    ap.add_argument("--fragments", type=int, default=20_000)
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--strains", type=int, default=64)
    ap.add_argument("--rate-ppm", type=int, default=3000)
    ap.add_argument("--h", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-c", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from miekki_amd import lib as L
    if args.lib:
        L._LIB_PATH = os.path.abspath(args.lib)
        have = C.CDLL(L._LIB_PATH)
        for name in [n for n in L.SIGNATURES if not hasattr(have, n)]:
            if not args.only_c:
                raise SystemExit(f"{args.lib} has no {name}")
            del L.SIGNATURES[name]
    import miekki_amd
    import synth
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, NF, thr = args.genomes, args.fragments, 200
    mi = 0.5 * thr
    ix = miekki_amd.Miekki(31, args.h, 8, 33, thr)
    ix.reserve(G)
    for g0 in range(0, G, 2048):
        ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
    L.check(lib.mk_sync(ix._h))
    say(f"{args.tag + ': ' if args.tag else ''}index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, "
        f"-k 31 -h {args.h}; {NF} fragments of 400 bases, thresholds (10, {mi}); {args.repeats} timed passes after one warm-up: min / median / max")
    d_tally = C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, 32 * G, C.byref(d_tally)))
    rng = np.random.default_rng(9)
    frags = []
    for _ in range(NF):
        g = int(rng.integers(0, G))
        frags.append(synth.strain_device(g, args.strains, args.rate_ppm, int(rng.integers(0, args.length - 400)), 400))
    m1 = [f[:150] for f in frags]
    m2 = [f[-150:].translate(_COMP)[::-1] for f in frags]

    def route(tag, make, n):
        qs = C.c_void_p()
        make(qs)

        def one():
            L.check(lib.mk_qset_invalidate(ix._h, qs))
            out = np.zeros((G, 4), np.uint64)
            L.check(lib.mk_tally_reset(ix._h, d_tally, G))
            L.check(lib.mk_qset_run_tally(ix._h, qs, 10, mi, d_tally, G))
            L.check(lib.mk_tally_read(ix._h, d_tally, G, out.ctypes.data))
            return out

        one()                                                    # warm-up: code objects, buffers
        ts, sk, sc = [], [], []
        for _ in range(args.repeats):
            ix.reset_stats()
            t = time.perf_counter()
            out = one()
            ts.append(time.perf_counter() - t)
            s = ix.stats()
            sk.append(s["sketch_ms"]); sc.append(s["scan_ms"])
        lib.mk_qset_free(ix._h, qs)
        say(f"  {tag}: {n} queries   sketch_ms {min(sk):6.3f} / {float(np.median(sk)):6.3f} / {max(sk):6.3f}   tally pass wall "
            f"{min(ts) * 1e3:6.1f} / {float(np.median(ts)) * 1e3:6.1f} / {max(ts) * 1e3:6.1f} ms (scan_ms {float(np.median(sc)):.1f})   "
            f"assigned {int(out[:, 2].sum())}, unique {int(out[:, 1].sum())}, listed {int(out[:, 0].sum())}")

    def single(reads):
        def make(qs):
            p, l = L.seq_arrays(reads)
            L.check(lib.mk_qset_upload(ix._h, p, l, len(reads), C.byref(qs)))
        return make

    def paired(qs):
        p1, l1 = L.seq_arrays(m1)
        p2, l2 = L.seq_arrays(m2)
        L.check(lib.mk_qset_upload_pairs(ix._h, p1, l1, p2, l2, NF, C.byref(qs)))

    if not args.only_c:
        route("(a) pairs of 2 x 150          ", paired, NF)
        route("(b) the mates as single reads ", single([m for p in zip(m1, m2) for m in p]), 2 * NF)
    route("(c) single reads of 300 bases ", single([f[:300] for f in frags]), NF)
    lib.mk_dev_free(ix._h, d_tally)
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
