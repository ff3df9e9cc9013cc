"""What does depth of coverage cost: the marks of a read set -- a compare-and-swap per value instead of the cover's OR -- and
the nine passes over the matrix that give covered, sum and median?  (recorded, not gated: profiles/sample_depth.txt)

The setup of tools/cover_rate.py (profiles/sample_cover.txt): 20,000 synthetic strain genomes in families of 64 at -k 31 -h 17,
reads of 1 kb cut from genomes drawn at random as ONE uploaded set, invalidated before every mark pass so that a pass is
complete (sketch, Bloom gate, marks).  A host clock around calls that end in a device wait, one warm-up and --repeats timed
passes (min / median / max), with the device's own event times (mk_stats.filter_ms) beside it:
  mark     mk_depth_reset + mk_qset_run_depth + mk_sync     with and without the plain load in front of the compare-and-swap
  cover    mk_cover_reset + mk_qset_run_cover + mk_sync     the same set: the OR the depth marks stand beside
  count    mk_cover_count                                   the yardstick of a pass: one bit lookup per fingerprint
  pass 0   mk_depth_profile with MIEKKI_DEPTH_STEPS=0, cells and saturated NULL: covered and sum
  all 9    mk_depth_profile, cells and saturated NULL; the eight bisection passes are the difference
  cells    mk_depth_profile with cells and saturated, less the line above
for 20,000 and 200,000 reads at 8 bits, and for the smaller set at 16 bits (-f 11, the same genomes: an 8 GiB table).

    python tools/depth_rate.py [--genomes 20000] [--out FILE]
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
    rng = np.random.default_rng(8)                               # (cover_rate.py's case 1)
    jobs = [(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(NMAX)]
    with multiprocessing.get_context("fork").Pool(args.workers) as pool:     # the reads first, in processes that never see the device
        reads = pool.map(cut, jobs, chunksize=2000)
    import miekki_amd
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(ix, fn):
        fn()                                                     # warm-up: code objects, buffers
        ts, dev = [], []
        for _ in range(args.repeats):
            ix.reset_stats()
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
            s = ix.stats()
            dev.append((s["sketch_ms"], s["filter_ms"]))
        return np.array(ts) * 1e3, np.array(dev)

    def mmm(a):
        return f"{np.min(a):8.3f} / {np.median(a):8.3f} / {np.max(a):8.3f}"

    def matrix_bytes(bits):
        return (1 << args.h) * ((G * (bits // 8) + 1023) // 1024 * 1024)

    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; reads of 1 kb "
        f"from genomes at random; {args.repeats} timed passes after one warm-up: min / median / max (ms)")
    for bits, sets in ((8, args.queries), (16, [min(args.queries)])):
        ix = miekki_amd.Miekki(31, args.h, bits, 33, 200)
        ix.reserve(G)
        for g0 in range(0, G, 2048):
            ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
        L.check(lib.mk_sync(ix._h))
        gbps, nbytes = C.c_double(0), C.c_uint64(0)
        L.check(lib.mk_probe_stream_read(ix._h, 5, C.byref(gbps), C.byref(nbytes)))
        floor_ms = matrix_bytes(bits) / (gbps.value * 1e9) * 1e3
        d_mult, d_seen = C.c_void_p(), C.c_void_p()
        L.check(lib.mk_dev_alloc(ix._h, lib.mk_depth_bytes(ix._h), C.byref(d_mult)))
        L.check(lib.mk_dev_alloc(ix._h, lib.mk_cover_bytes(ix._h), C.byref(d_seen)))
        say(f"{bits}-bit fingerprints: matrix {matrix_bytes(bits)} bytes, depth table {lib.mk_depth_bytes(ix._h)} bytes, cover table {lib.mk_cover_bytes(ix._h)} bytes; "
            f"mk_probe_stream_read {gbps.value:.0f} GB/s = {floor_ms:.3f} ms per read of the matrix; to the host per profile: {16 * G + 16} bytes")
        depth = np.zeros(G, np.dtype([("sum", np.uint64), ("covered", np.uint32), ("median", np.uint32)]))
        cov, cells, sat = np.zeros(G, np.uint32), C.c_uint64(0), C.c_uint64(0)
        for NQ in sets:
            ptrs, lens = L.seq_arrays(reads[:NQ])
            qs = C.c_void_p()
            L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))

            def mark():
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                L.check(lib.mk_depth_reset(ix._h, d_mult))
                L.check(lib.mk_qset_run_depth(ix._h, qs, d_mult))
                L.check(lib.mk_sync(ix._h))

            def cover():
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                L.check(lib.mk_cover_reset(ix._h, d_seen))
                L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen))
                L.check(lib.mk_sync(ix._h))

            def count():
                L.check(lib.mk_cover_count(ix._h, d_seen, cov.ctypes.data, None))

            def passes():
                L.check(lib.mk_depth_profile(ix._h, d_mult, depth.ctypes.data, None, None))

            def with_cells():
                L.check(lib.mk_depth_profile(ix._h, d_mult, depth.ctypes.data, C.byref(cells), C.byref(sat)))

            say(f"  {NQ} reads")
            for flt in ("0", "1"):
                os.environ["MIEKKI_DEPTH_FILTER"] = flt
                ts, dev = timed(ix, mark)
                say(f"    depth marks, filter {flt}: wall {mmm(ts)}   device: sketch {np.median(dev[:, 0]):.3f}  mark_ms {mmm(dev[:, 1])}")
            del os.environ["MIEKKI_DEPTH_FILTER"]
            ts, dev = timed(ix, cover)
            say(f"    cover marks (filter 1) : wall {mmm(ts)}   device: sketch {np.median(dev[:, 0]):.3f}  mark_ms {mmm(dev[:, 1])}")
            ts, dev = timed(ix, count)
            count_ms = float(np.median(dev[:, 1]))
            say(f"    cover count, no cells  : wall {mmm(ts)}   device: {mmm(dev[:, 1])}   = {count_ms / floor_ms:.2f} x the probe's floor")
            os.environ["MIEKKI_DEPTH_STEPS"] = "0"
            ts, dev = timed(ix, passes)
            pass0 = float(np.median(dev[:, 1]))
            say(f"    depth pass 0           : wall {mmm(ts)}   device: {mmm(dev[:, 1])}   = {pass0 / count_ms:.2f} x the count pass")
            del os.environ["MIEKKI_DEPTH_STEPS"]
            ts, dev = timed(ix, passes)
            all9 = float(np.median(dev[:, 1]))
            say(f"    depth, all 9 passes    : wall {mmm(ts)}   device: {mmm(dev[:, 1])}   the 8 bisection passes: {all9 - pass0:.3f} = {(all9 - pass0) / 8:.3f} each; "
                f"all = {all9 / (9 * count_ms):.2f} x nine count passes")
            ts, dev = timed(ix, with_cells)
            say(f"    ... with cells         : wall {mmm(ts)}   device: {mmm(dev[:, 1])}   the reduction over the table: {float(np.median(dev[:, 1])) - all9:.3f}")
            d = depth[depth["covered"] > 0]
            say(f"      cells {cells.value} of {(1 << args.h) << bits}, at 255: {sat.value}; genomes covered {len(d)}; median of the medians {int(np.median(d['median'])) if len(d) else 0}, "
                f"largest {int(d['median'].max()) if len(d) else 0}; mean depth sum / covered: median {float(np.median(d['sum'] / d['covered'])) if len(d) else 0:.2f}")
            lib.mk_qset_free(ix._h, qs)
        lib.mk_dev_free(ix._h, d_seen)
        lib.mk_dev_free(ix._h, d_mult)
        ix.close()
    say("(tools/depth_rate.py; host clock around calls that end in a device wait; one MI355X.)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
