"""What does the profile of a read set cost, summed on the device or on the host?  (recorded, not gated:
profiles/query_tally.txt)

The index of profiles/r8_query_list.txt -- 20,000 synthetic strain genomes in families of 64 at -h 17 -- and 20,000 reads
of 1 kb as ONE uploaded set, invalidated before every pass so that a pass is complete (sketch, Bloom gate, scan, walk).
Two routes to the same four counters per genome, each timed by a host clock around calls that end in a device wait, one
warm-up and --repeats timed passes (min / median / max):
  (t) mk_tally_reset + mk_qset_run_tally + mk_tally_read          one scan, one walk, 32 bytes per genome to the host
  (l) mk_qset_run_list(MK_LIST_CANDIDATES) + mk_qset_run_list(1)  the only route without the tally: two scans, the lists
      + a numpy sum over the records                              of every read to the host, then the sum
and two read sets:
  case 1  reads cut from genomes drawn at random: the adds spread over the index
  case 2  reads all cut from ONE genome: every wave adds to the same 64 rows of counters -- the worst case for the atomics
The two routes' counters are compared before anything is reported.

    python tools/tally_rate.py [--genomes 20000] [--queries 20000] [--out FILE]
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
        f"{NQ} reads of 1 kb, thresholds (10, {mi}); {args.repeats} timed passes after one warm-up: min / median / max")
    d_tally = C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, 32 * G, C.byref(d_tally)))

    def timed(fn):
        fn()                                                     # warm-up: code objects, buffers
        ts, dev = [], None
        for _ in range(args.repeats):
            ix.reset_stats()
            t = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t)
            s = ix.stats()
            dev = (s["sketch_ms"], s["scan_ms"], s["filter_ms"])
        return (min(ts), float(np.median(ts)), max(ts)), dev, out

    def case(name, reads):
        ptrs, lens = L.seq_arrays(reads)
        qs = C.c_void_p()
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))

        def route_t():
            L.check(lib.mk_qset_invalidate(ix._h, qs))
            out = np.zeros((G, 4), np.uint64)
            L.check(lib.mk_tally_reset(ix._h, d_tally, G))
            L.check(lib.mk_qset_run_tally(ix._h, qs, 10, mi, d_tally, G))
            L.check(lib.mk_tally_read(ix._h, d_tally, G, out.ctypes.data))
            return out, 32 * G

        def lists(nresults):
            hl = C.c_void_p()
            L.check(lib.mk_qset_run_list(ix._h, qs, nresults, 10, mi, C.byref(hl)))
            off = np.ctypeslib.as_array(lib.mk_hitlist_offsets(hl), (NQ + 1,)).copy()
            rec = np.zeros(int(off[NQ]), HIT)
            if len(rec):
                C.memmove(rec.ctypes.data, lib.mk_hitlist_hits(hl), rec.nbytes)
            lib.mk_hitlist_free(hl)
            return off, rec

        def route_l():
            L.check(lib.mk_qset_invalidate(ix._h, qs))
            off, rec = lists(L.LIST_CANDIDATES)
            L.check(lib.mk_qset_invalidate(ix._h, qs))
            off1, rec1 = lists(1)
            out = np.zeros((G, 4), np.uint64)
            out[:, 0] = np.bincount(rec["genome"], minlength=G)
            alone = np.flatnonzero(np.diff(off) == 1)
            out[:, 1] = np.bincount(rec["genome"][off[alone]], minlength=G)
            out[:, 2] = np.bincount(rec1["genome"], minlength=G)
            out[:, 3] = np.bincount(rec1["genome"], weights=rec1["matches"], minlength=G).astype(np.uint64)
            # per chunk and list call: two offsets per query and its active partitions beside the hits
            return out, 24 * (len(rec) + len(rec1)) + 2 * (20 * NQ + 16)

        t_ts, t_dev, (t_out, t_bytes) = timed(route_t)
        l_ts, l_dev, (l_out, l_bytes) = timed(route_l)
        if not np.array_equal(t_out, l_out):
            raise SystemExit(f"{name}: the two routes disagree")
        say(f"{name}: {int(t_out[:, 0].sum())} (read, genome) pairs listed, {int((t_out[:, 0] > 0).sum())} genomes listed, "
            f"{int(t_out[:, 2].sum())} reads assigned to {int((t_out[:, 2] > 0).sum())} genomes; both routes agree")
        for tag, ts, dev, nbytes in (("(t) tally on the device      ", t_ts, t_dev, t_bytes), ("(l) two list passes + host sum", l_ts, l_dev, l_bytes)):
            say(f"  {tag}: wall {ts[0] * 1e3:7.1f} / {ts[1] * 1e3:7.1f} / {ts[2] * 1e3:7.1f} ms   device ms: sketch {dev[0]:.1f} scan {dev[1]:.1f} "
                f"filter {dev[2]:.2f}   to the host: {nbytes} bytes")
        say(f"  (l) / (t): wall {l_ts[1] / t_ts[1]:.2f}, filter_ms {l_dev[2] / max(t_dev[2], 1e-9):.2f}")
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
    lib.mk_dev_free(ix._h, d_tally)
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
