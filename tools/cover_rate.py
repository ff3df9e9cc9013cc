"""What does breadth of coverage cost: the marks of a read set, and the one pass over the matrix that counts?  (recorded, not
gated: profiles/sample_cover.txt)

The index of profiles/query_tally.txt -- 20,000 synthetic strain genomes in families of 64 at -k 31 -h 17 -- and reads of
1 kb as ONE uploaded set, invalidated before every pass so that a pass is complete (sketch, Bloom gate, marks).  Everything
is timed by a host clock around calls that end in a device wait, one warm-up and --repeats timed passes (min / median /
max), with the device's own event times (mk_stats) beside it:
  mark    mk_cover_reset + mk_qset_run_cover + mk_sync      with and without the plain load in front of the atomic
  count   mk_cover_count                                    against matrix bytes / mk_probe_stream_read's rate
  tally   mk_tally_reset + mk_qset_run_tally + mk_tally_read, the same reads, for context: it answers another question
for 20,000 and for 200,000 reads of two kinds:
  case 1  reads cut from genomes drawn at random
  case 2  reads all cut from ONE genome: every wave ORs into the same words
and the 16-bit table (-f 11, the same genomes): its bytes and its count pass.

    python tools/cover_rate.py [--genomes 20000] [--out FILE]
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
    G, thr, NMAX = args.genomes, 200, max(args.queries)
    mi = 0.5 * thr
    # the reads first, in worker processes that never see the device
    rng = np.random.default_rng(8)
    one_g = G // 2 + 7
    jobs1 = [(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(NMAX)]
    jobs2 = [(one_g, args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(NMAX)]
    with multiprocessing.get_context("fork").Pool(args.workers) as pool:
        spread = pool.map(cut, jobs1, chunksize=2000)
        one = pool.map(cut, jobs2, chunksize=2000)
    import miekki_amd
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def build(bits):
        ix = miekki_amd.Miekki(31, args.h, bits, 33, thr)
        ix.reserve(G)
        for g0 in range(0, G, 2048):
            ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
        L.check(lib.mk_sync(ix._h))
        return ix

    def timed(ix, fn):
        fn()                                                     # warm-up: code objects, buffers
        ts, dev = [], []
        for _ in range(args.repeats):
            ix.reset_stats()
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
            s = ix.stats()
            dev.append((s["sketch_ms"], s["scan_ms"], s["filter_ms"]))
        return np.array(ts) * 1e3, np.array(dev)

    def mmm(a):
        return f"{np.min(a):8.3f} / {np.median(a):8.3f} / {np.max(a):8.3f}"

    def matrix_bytes(bits):
        return (1 << args.h) * ((G * (bits // 8) + 1023) // 1024 * 1024)

    ix = build(8)
    P = 1 << args.h
    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; "
        f"matrix {matrix_bytes(8)} bytes; reads of 1 kb; {args.repeats} timed passes after one warm-up: min / median / max (ms)")
    gbps, nbytes = C.c_double(0), C.c_uint64(0)
    L.check(lib.mk_probe_stream_read(ix._h, 5, C.byref(gbps), C.byref(nbytes)))
    floor_ms = matrix_bytes(8) / (gbps.value * 1e9) * 1e3
    say(f"mk_probe_stream_read: {gbps.value:.0f} GB/s over {nbytes.value} bytes: one read of the matrix at that rate = {floor_ms:.3f} ms")
    tab_bytes = lib.mk_cover_bytes(ix._h)
    d_seen, d_tally = C.c_void_p(), C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, tab_bytes, C.byref(d_seen)))
    L.check(lib.mk_dev_alloc(ix._h, 32 * G, C.byref(d_tally)))
    cov, cells = np.zeros(G, np.uint32), C.c_uint64(0)
    say(f"table: {tab_bytes} bytes at 8 bits; to the host per count: {4 * G + 8} bytes")
    count_medians = []
    for name, reads in ((f"case 1, reads from genomes at random", spread), (f"case 2, reads from genome {one_g} alone", one)):
        for NQ in args.queries:
            ptrs, lens = L.seq_arrays(reads[:NQ])
            qs = C.c_void_p()
            L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))

            def mark():
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                L.check(lib.mk_cover_reset(ix._h, d_seen))
                L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen))
                L.check(lib.mk_sync(ix._h))

            def count():
                L.check(lib.mk_cover_count(ix._h, d_seen, cov.ctypes.data, C.byref(cells)))

            def tally():
                out = np.zeros((G, 4), np.uint64)
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                L.check(lib.mk_tally_reset(ix._h, d_tally, G))
                L.check(lib.mk_qset_run_tally(ix._h, qs, 10, mi, d_tally, G))
                L.check(lib.mk_tally_read(ix._h, d_tally, G, out.ctypes.data))

            say(f"{name}, {NQ} reads")
            for flt in ("0", "1"):
                os.environ["MIEKKI_COVER_FILTER"] = flt
                ts, dev = timed(ix, mark)
                say(f"  mark, filter {flt}: wall {mmm(ts)}   device: sketch {np.median(dev[:, 0]):.3f}  mark_ms {mmm(dev[:, 2])}")
            del os.environ["MIEKKI_COVER_FILTER"]
            ts, dev = timed(ix, count)
            count_medians.append(float(np.median(dev[:, 2])))
            say(f"  count           : wall {mmm(ts)}   device: count_ms {mmm(dev[:, 2])}   = {np.median(dev[:, 2]) / floor_ms:.2f} x the probe's floor, "
                f"{matrix_bytes(8) / np.median(dev[:, 2]) / 1e6:.0f} GB/s")
            say(f"    cells {cells.value} of {P << 8} ({cells.value / (P << 8):.4f}: the chance floor of an unrelated genome), genomes covered {int((cov > 0).sum())}, "
                f"largest covered / sketch_size {float((cov / np.maximum(ix.sketch_size, 1)).max()):.3f}, median {float(np.median(cov / np.maximum(ix.sketch_size, 1))):.4f}")
            ts, dev = timed(ix, tally)
            say(f"  tally (context) : wall {mmm(ts)}   device: sketch {np.median(dev[:, 0]):.1f} scan {np.median(dev[:, 1]):.1f} filter {np.median(dev[:, 2]):.2f}")
            lib.mk_qset_free(ix._h, qs)
    say(f"count_ms medians over the {len(count_medians)} read sets: " + ", ".join(f"{m:.3f}" for m in count_medians))
    lib.mk_dev_free(ix._h, d_tally)
    lib.mk_dev_free(ix._h, d_seen)
    ix.close()

    ix = build(16)
    tab_bytes = lib.mk_cover_bytes(ix._h)
    L.check(lib.mk_probe_stream_read(ix._h, 5, C.byref(gbps), C.byref(nbytes)))
    floor_ms = matrix_bytes(16) / (gbps.value * 1e9) * 1e3
    say(f"16-bit fingerprints (-f 11), the same genomes: matrix {matrix_bytes(16)} bytes, table {tab_bytes} bytes; to the host per count: {4 * G + 8} bytes; "
        f"probe {gbps.value:.0f} GB/s = {floor_ms:.3f} ms per read of the matrix")
    L.check(lib.mk_dev_alloc(ix._h, tab_bytes, C.byref(d_seen)))
    NQ = min(args.queries)
    ptrs, lens = L.seq_arrays(spread[:NQ])
    qs = C.c_void_p()
    L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))

    def mark16():
        L.check(lib.mk_qset_invalidate(ix._h, qs))
        L.check(lib.mk_cover_reset(ix._h, d_seen))
        L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen))
        L.check(lib.mk_sync(ix._h))

    def count16():
        L.check(lib.mk_cover_count(ix._h, d_seen, cov.ctypes.data, C.byref(cells)))

    ts, dev = timed(ix, mark16)
    say(f"  case 1, {NQ} reads: reset + mark: wall {mmm(ts)}   device: sketch {np.median(dev[:, 0]):.3f}  mark_ms {mmm(dev[:, 2])}  (the reset clears {tab_bytes} bytes)")
    ts, dev = timed(ix, count16)
    say(f"  count           : wall {mmm(ts)}   device: count_ms {mmm(dev[:, 2])}   = {np.median(dev[:, 2]) / floor_ms:.2f} x the probe's floor, "
        f"{matrix_bytes(16) / np.median(dev[:, 2]) / 1e6:.0f} GB/s (cells included: a popcount of the table)")
    say(f"    cells {cells.value} of {P << 16}, genomes covered {int((cov > 0).sum())}")
    lib.mk_qset_free(ix._h, qs)
    lib.mk_dev_free(ix._h, d_seen)
    ix.close()
    say("(tools/cover_rate.py; host clock around calls that end in a device wait; one MI355X.)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
