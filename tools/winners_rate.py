"""What does the winner-takes-all pass cost beside the count pass it follows?  (recorded, not gated: profiles/sample_winners.txt)

The index of profiles/sample_cover.txt -- 20,000 synthetic strain genomes in families of 64 at -k 31 -h 17 -- and reads of 1 kb
marked into a cover table once per read set; then, on that table, from the same run, one warm-up and --repeats timed passes
each (min / median / max), a host clock around calls that end in a device wait with the device's own event times (mk_stats
filter_ms) beside it:
  count     mk_cover_count                           the yardstick: its kernel is the parent's
  winners   mk_cover_winners                         count, the order sorted on the host, the win pass
  assign    mk_cover_assign with that order          the win pass with its copies (rank and order up, won down) and the
                                                     permutation check; its device time is the win kernel alone
  host      winners wall - count wall - assign wall  the sort
for 20,000 and for 200,000 reads of two kinds at one byte:
  case 1  reads cut from genomes drawn at random: winners all over the index
  case 2  reads all cut from ONE genome: its family wins every cell -- the adds to `won` hit a few addresses
and for case 1 at two bytes (-f 11, the same genomes).  Switches, each against the default: MIEKKI_WIN_FILTER=0 (every live,
seen fingerprint does its LDS atomic), and at two bytes MIEKKI_WIN_TOUCHED=0 (the whole range read out and cleared per row
instead of the touched slots) and MIEKKI_WIN_VALUES (ranges of 4,096 / 16,384 / 32,768 values: 16 / 4 / 2 passes per row).

    python tools/winners_rate.py [--genomes 20000] [--out FILE]
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
    ap.add_argument("--queries", type=int, nargs="+", default=[20_000, 200_000])
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--strains", type=int, default=64)
    ap.add_argument("--rate-ppm", type=int, default=3000)
    ap.add_argument("--h", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G, NMAX = args.genomes, max(args.queries)
    # the reads first, in worker processes that never see the device
    rng = np.random.default_rng(8)
    one_g = G // 2 + 7
    jobs1 = [(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(NMAX)]
    jobs2 = [(one_g, args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(NMAX)]
    with multiprocessing.get_context("fork").Pool(args.workers) as pool:
        spread = pool.map(cut, jobs1, chunksize=2000)
        one = pool.map(cut, jobs2, chunksize=2000)
    import miekki_amd
    import winners_ref as wr
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def build(bits):
        ix = miekki_amd.Miekki(31, args.h, bits, 33, 200)
        ix.reserve(G)
        for g0 in range(0, G, 2048):
            ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
        L.check(lib.mk_sync(ix._h))
        return ix

    def timed(ix, fn, env=None):
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

    def mmm(a):
        return f"{np.min(a):8.3f} / {np.median(a):8.3f} / {np.max(a):8.3f}"

    def matrix_bytes(bits):
        return (1 << args.h) * ((G * (bits // 8) + 1023) // 1024 * 1024)

    def one_set(ix, bits, d_seen, name, reads, switches):
        NQ = len(reads)
        ptrs, lens = L.seq_arrays(reads)
        qs = C.c_void_p()
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))
        L.check(lib.mk_cover_reset(ix._h, d_seen))
        L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen))
        L.check(lib.mk_sync(ix._h))
        lib.mk_qset_free(ix._h, qs)
        cov, won = np.zeros(G, np.uint32), np.zeros(G, np.uint32)
        cells, claimed = C.c_uint64(0), C.c_uint64(0)

        def count():
            L.check(lib.mk_cover_count(ix._h, d_seen, cov.ctypes.data, C.byref(cells)))

        def winners():
            L.check(lib.mk_cover_winners(ix._h, d_seen, cov.ctypes.data, won.ctypes.data, C.byref(cells), C.byref(claimed)))

        say(f"{name}, {NQ} reads")
        tc, dc = timed(ix, count)
        say(f"  count              : wall {mmm(tc)}   device: count_ms {mmm(dc)}")
        tw, dw = timed(ix, winners)
        order = wr.order(cov, ix.sketch_size).astype(np.uint32)
        got = np.zeros(G, np.uint32)

        def assign():
            L.check(lib.mk_cover_assign(ix._h, d_seen, order.ctypes.data, got.ctypes.data, None))

        ta, da = timed(ix, assign)
        assert (got == won).all() and int(won.sum()) == claimed.value
        ratio = np.median(da) / np.median(dc)
        say(f"  winners            : wall {mmm(tw)}   device: count + win {mmm(dw)}")
        say(f"  assign             : wall {mmm(ta)}   device: win_ms {mmm(da)}   = {ratio:.2f} x the count pass, "
            f"{matrix_bytes(bits) / np.median(da) / 1e6:.0f} GB/s over the matrix bytes")
        say(f"    host sort (winners - count - assign, medians of wall): {np.median(tw) - np.median(tc) - np.median(ta):.3f} ms; "
            f"assign's copies and permutation check (wall - device): {np.median(ta) - np.median(da):.3f} ms for {12 * G} bytes")
        ss = np.maximum(ix.sketch_size, 1)
        top = np.sort(won)[::-1]
        say(f"    cells {cells.value}, claimed {claimed.value} (= adds to won), genomes covered {int((cov > 0).sum())}, genomes that win {int((won > 0).sum())}, "
            f"largest won {int(top[0])}, the 64 largest hold {int(top[:64].sum())}; median covered / sketch {float(np.median(cov / ss)):.4f}, median won / sketch {float(np.median(won / ss)):.4f}")
        for label, env in switches:
            t, d = timed(ix, assign, env)
            assert (got == won).all()
            say(f"  assign, {label:<28}: device: win_ms {mmm(d)}   = {np.median(d) / np.median(da):.2f} x the default")
        return float(np.median(dc)), float(np.median(da))

    ix = build(8)
    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; "
        f"matrix {matrix_bytes(8)} bytes; reads of 1 kb; {args.repeats} timed passes after one warm-up: min / median / max (ms)")
    d_seen = C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, lib.mk_cover_bytes(ix._h), C.byref(d_seen)))
    pairs = []
    for name, reads in (("case 1, reads from genomes at random", spread), (f"case 2, reads from genome {one_g} alone", one)):
        for NQ in args.queries:
            pairs.append(one_set(ix, 8, d_seen, name, reads[:NQ], [("MIEKKI_WIN_FILTER=0", {"MIEKKI_WIN_FILTER": "0"})]))
    say("count_ms / win_ms medians over the read sets: " + ", ".join(f"{a:.3f} / {b:.3f}" for a, b in pairs))
    lib.mk_dev_free(ix._h, d_seen)
    ix.close()

    ix = build(16)
    say(f"16-bit fingerprints (-f 11), the same genomes: matrix {matrix_bytes(16)} bytes, table {lib.mk_cover_bytes(ix._h)} bytes")
    L.check(lib.mk_dev_alloc(ix._h, lib.mk_cover_bytes(ix._h), C.byref(d_seen)))
    switches = [("MIEKKI_WIN_TOUCHED=0", {"MIEKKI_WIN_TOUCHED": "0"}),
                ("MIEKKI_WIN_FILTER=0", {"MIEKKI_WIN_FILTER": "0"}),
                ("MIEKKI_WIN_VALUES=4096", {"MIEKKI_WIN_VALUES": "4096"}),
                ("MIEKKI_WIN_VALUES=32768", {"MIEKKI_WIN_VALUES": "32768"}),
                ("VALUES=32768, TOUCHED=0", {"MIEKKI_WIN_VALUES": "32768", "MIEKKI_WIN_TOUCHED": "0"})]
    pairs = [one_set(ix, 16, d_seen, "case 1, reads from genomes at random", spread[:NQ], switches) for NQ in args.queries]
    say("count_ms / win_ms medians over the read sets: " + ", ".join(f"{a:.3f} / {b:.3f}" for a, b in pairs))
    lib.mk_dev_free(ix._h, d_seen)
    ix.close()
    say("(tools/winners_rate.py; host clock around calls that end in a device wait; one MI355X.)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
