"""What does the greedy gather cost, and which way of keeping `rem` current wins?  (recorded, not gated: profiles/sample_gather.txt)

The index of profiles/sample_cover.txt -- 20,000 synthetic strain genomes in families of 64 at -k 31 -h 17 -- and its 20,000 reads
of 1 kb cut from genomes drawn at random, marked into a cover table once; then on that table, at both fingerprint widths:
  count     mk_cover_count                           the yardstick: the parent's count pass, re-measured here.  That figure
                                                     times the number of picks is the only route that existed before (a host
                                                     loop, without its two table copies over PCIe per pick)
  gather    mk_cover_gather, min_new 10, no cap      pick + take + strike per round, 32 rounds queued per host wait
  recount   the same with MIEKKI_GATHER_RECOUNT=1    pick + take + the count pass over the struck table per round
  rounds=1  the same with MIEKKI_GATHER_ROUNDS=1     the strike route with a host wait after every round
each with the picks, the total (host clock around a call that ends in a device wait; mk_stats filter_ms beside it), the time per
round, and the bytes the strike steps read (the sum of fresh x the row's bytes) against picks x matrix bytes.  The picks of the
three routes must be identical.  The recount leg is timed once (it takes picks x count pass).

The split between the pick, take and strike kernels comes from a run of its own under the profiler's kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gather_rate.py --once [--bits 8]
which builds, marks, and runs one warm-up and one gather and nothing else.

    python tools/gather_rate.py [--genomes 20000] [--out FILE]
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
    ap.add_argument("--min-new", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--bits", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--once", action="store_true", help="one warm-up and one gather per width and nothing else: for a profiler run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G = args.genomes
    rng = np.random.default_rng(8)
    jobs = [(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(args.queries)]
    with multiprocessing.get_context("fork").Pool(args.workers) as pool:     # (worker processes that never see the device)
        reads = pool.map(cut, jobs, chunksize=2000)
    import miekki_amd
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def mmm(a):
        return f"{np.min(a):9.3f} / {np.median(a):9.3f} / {np.max(a):9.3f}"

    for bits in args.bits:
        ix = miekki_amd.Miekki(31, args.h, bits, 33, 200)
        ix.reserve(G)
        for g0 in range(0, G, 2048):
            ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
        L.check(lib.mk_sync(ix._h))
        row_bytes = (G * (bits // 8) + 1023) // 1024 * 1024
        matrix = (1 << args.h) * row_bytes
        d_seen, qs = C.c_void_p(), C.c_void_p()
        L.check(lib.mk_dev_alloc(ix._h, lib.mk_cover_bytes(ix._h), C.byref(d_seen)))
        ptrs, lens = L.seq_arrays(reads)
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, len(reads), C.byref(qs)))
        L.check(lib.mk_cover_reset(ix._h, d_seen))
        L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen))
        L.check(lib.mk_sync(ix._h))
        lib.mk_qset_free(ix._h, qs)
        say(f"{bits}-bit fingerprints: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; "
            f"matrix {matrix} bytes, table {lib.mk_cover_bytes(ix._h)} bytes; {len(reads)} reads of 1 kb; min_new {args.min_new}; "
            f"min / median / max (ms)")
        cov = np.zeros(G, np.uint32)
        picks = np.zeros(G, miekki_amd.Miekki.PICK_DTYPE)
        n, cells, explained = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)

        def count():
            L.check(lib.mk_cover_count(ix._h, d_seen, cov.ctypes.data, C.byref(cells)))

        def gather():
            L.check(lib.mk_cover_gather(ix._h, d_seen, None, args.min_new, 0, picks.ctypes.data, C.byref(n), C.byref(cells), C.byref(explained)))

        def timed(fn, repeats, env=None, warm=True):
            for k, v in (env or {}).items():
                os.environ[k] = v
            try:
                if warm:
                    fn()
                ts, dev = [], []
                for _ in range(repeats):
                    ix.reset_stats()
                    t = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t)
                    dev.append(ix.stats()["filter_ms"])
            finally:
                for k in env or {}:
                    del os.environ[k]
            return np.array(ts) * 1e3, np.array(dev)

        if args.once:
            timed(gather, 1)
            say(f"  once: {n.value} picks, explained {explained.value} of {cells.value} cells")
        else:
            tc, dc = timed(count, args.repeats)
            say(f"  count              : wall {mmm(tc)}   device {mmm(dc)}")
            tg, dg = timed(gather, args.repeats)
            base = picks[:n.value].copy()
            rounds = n.value + 1                                          # (the round that stops the loop runs its pick and take steps)
            struck = int(base["fresh"].astype(np.int64).sum()) * row_bytes
            say(f"  gather             : wall {mmm(tg)}   device {mmm(dg)}   {n.value} picks, explained {explained.value} of {cells.value} cells")
            say(f"    per round: wall {np.median(tg) / rounds * 1e3:.2f} us, device {np.median(dg) / rounds * 1e3:.2f} us; the count pass per pick would be "
                f"{np.median(dc) * n.value:.1f} ms = {np.median(dc) * n.value / np.median(tg):.1f} x the gather's wall")
            say(f"    strike steps read {struck} bytes = {struck / matrix:.2f} matrices, against picks x matrix = {n.value * matrix} bytes "
                f"({n.value * matrix / max(struck, 1):.0f} x); fresh: first {int(base['fresh'][0]) if n.value else 0}, median "
                f"{int(np.median(base['fresh'])) if n.value else 0}, last {int(base['fresh'][-1]) if n.value else 0}")
            t1, d1 = timed(gather, args.repeats, {"MIEKKI_GATHER_ROUNDS": "1"})
            assert np.array_equal(picks[:n.value], base)
            say(f"  gather, ROUNDS=1   : wall {mmm(t1)}   device {mmm(d1)}   per round: wall {np.median(t1) / rounds * 1e3:.2f} us")
            tr, dr_ = timed(gather, 1, {"MIEKKI_GATHER_RECOUNT": "1"}, warm=False)
            assert np.array_equal(picks[:n.value], base)
            say(f"  gather, RECOUNT=1  : wall {mmm(tr)}   device {mmm(dr_)}   per round: wall {np.median(tr) / rounds * 1e3:.2f} us "
                f"= {np.median(tr) / np.median(tg):.1f} x the strike route")
        lib.mk_dev_free(ix._h, d_seen)
        ix.close()
    say("(tools/gather_rate.py; host clock around calls that end in a device wait; one MI355X.)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
