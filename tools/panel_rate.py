"""Does a panel pay: eight samples through one table and ONE pass over the matrix (mk_qset_run_panel, mk_panel_count) against the
same eight through the cover that exists, a table and a pass each (mk_qset_run_cover, mk_cover_count)?  (recorded, not gated:
profiles/sample_panel.txt)

The index of profiles/sample_cover.txt -- 20,000 synthetic strain genomes in families of 64 at -k 31 -h 17, with 8-bit (-f 3)
and 16-bit (-f 11) fingerprints -- and eight samples of reads of 1 kb cut from genomes drawn at random, one uploaded set each,
invalidated before every mark pass so that a pass is complete (sketch, Bloom gate, marks).  Everything is timed by a host
clock around calls that end in a device wait, one warm-up and --repeats timed passes (min / median / max), with the device's
own event times (mk_stats.filter_ms) beside it; the two sides of a comparison alternate inside one loop, so that neither has
the warmer machine:
  mark    mk_panel_reset + 8 x mk_qset_run_panel + mk_sync   against   8 x (mk_cover_reset + mk_qset_run_cover) + mk_sync
  count   mk_panel_count(.., 8)                              against   8 x mk_cover_count
  one     mk_panel_count(.., 1), and the panel's marks with MIEKKI_PANEL_FILTER=0 and 1
and the counts of both sides are compared before anything is reported.

    python tools/panel_rate.py [--genomes 20000] [--reads 20000] [--out FILE]
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
SLOTS = 8


def cut(job):
    import synth
    g, strains, ppm, off = job
    return synth.strain_device(g, strains, ppm, off, 1000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=20_000)
    ap.add_argument("--reads", type=int, default=20_000, help="reads per sample")
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--strains", type=int, default=64)
    ap.add_argument("--rate-ppm", type=int, default=3000)
    ap.add_argument("--h", type=int, default=17)
    ap.add_argument("--widths", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    G, NQ = args.genomes, args.reads
    # the reads first, in worker processes that never see the device
    rng = np.random.default_rng(8)
    jobs = [(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000))) for _ in range(SLOTS * NQ)]
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

    def timed_pair(ix, fns):
        """the functions in turn, one warm-up round and args.repeats timed ones: per function (wall ms, filter_ms)"""
        for fn in fns:
            fn()
        wall, dev = [[] for _ in fns], [[] for _ in fns]
        for _ in range(args.repeats):
            for i, fn in enumerate(fns):
                ix.reset_stats()
                t = time.perf_counter()
                fn()
                wall[i].append((time.perf_counter() - t) * 1e3)
                dev[i].append(ix.stats()["filter_ms"])
        return [(np.array(w), np.array(d)) for w, d in zip(wall, dev)]

    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; {SLOTS} samples of {NQ} reads of 1 kb "
        f"from genomes at random; {args.repeats} timed passes after one warm-up, the two sides in turn: min / median / max (ms)")
    for bits in args.widths:
        ix = miekki_amd.Miekki(31, args.h, bits, 33, 200)
        ix.reserve(G)
        for g0 in range(0, G, 2048):
            ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
        L.check(lib.mk_sync(ix._h))
        matrix = (1 << args.h) * ((G * (bits // 8) + 1023) // 1024 * 1024)
        gbps, nbytes = C.c_double(0), C.c_uint64(0)
        L.check(lib.mk_probe_stream_read(ix._h, 5, C.byref(gbps), C.byref(nbytes)))
        floor_ms = matrix / (gbps.value * 1e9) * 1e3
        panel_bytes, cover_bytes = lib.mk_panel_bytes(ix._h), lib.mk_cover_bytes(ix._h)
        say(f"{bits}-bit fingerprints (-f {bits - 5}): matrix {matrix} bytes, panel table {panel_bytes} bytes, cover table {cover_bytes} bytes each; "
            f"probe {gbps.value:.0f} GB/s = {floor_ms:.3f} ms per read of the matrix")
        d_panel = C.c_void_p()
        L.check(lib.mk_dev_alloc(ix._h, panel_bytes, C.byref(d_panel)))
        d_seen = [C.c_void_p() for _ in range(SLOTS)]
        for d in d_seen:
            L.check(lib.mk_dev_alloc(ix._h, cover_bytes, C.byref(d)))
        sets = []
        for s in range(SLOTS):
            ptrs, lens = L.seq_arrays(reads[s * NQ:(s + 1) * NQ])
            qs = C.c_void_p()
            L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))
            sets.append(qs)
        pcov, pcells = np.zeros((SLOTS, G), np.uint32), np.zeros(SLOTS, np.uint64)
        ccov, ccells = np.zeros((SLOTS, G), np.uint32), np.zeros(SLOTS, np.uint64)

        def mark_panel():
            L.check(lib.mk_panel_reset(ix._h, d_panel))
            for s, qs in enumerate(sets):
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                L.check(lib.mk_qset_run_panel(ix._h, qs, s, d_panel))
            L.check(lib.mk_sync(ix._h))

        def mark_cover():
            for s, qs in enumerate(sets):
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                L.check(lib.mk_cover_reset(ix._h, d_seen[s]))
                L.check(lib.mk_qset_run_cover(ix._h, qs, d_seen[s]))
            L.check(lib.mk_sync(ix._h))

        def count_panel():
            L.check(lib.mk_panel_count(ix._h, d_panel, SLOTS, pcov.ctypes.data, pcells.ctypes.data))

        def count_one():
            L.check(lib.mk_panel_count(ix._h, d_panel, 1, pcov.ctypes.data, pcells.ctypes.data))

        def count_cover():
            for s in range(SLOTS):
                n = C.c_uint64(0)
                L.check(lib.mk_cover_count(ix._h, d_seen[s], ccov[s].ctypes.data, C.byref(n)))
                ccells[s] = n.value

        (pw, pd), (cw, cd) = timed_pair(ix, [mark_panel, mark_cover])
        say(f"  mark  panel, 8 samples into one table : wall {mmm(pw)}   device: mark_ms {mmm(pd)}")
        say(f"  mark  cover, 8 samples, a table each  : wall {mmm(cw)}   device: mark_ms {mmm(cd)}")
        for flt in ("0", "1"):
            os.environ["MIEKKI_PANEL_FILTER"] = flt
            ((w, d),) = timed_pair(ix, [mark_panel])
            say(f"  mark  panel, MIEKKI_PANEL_FILTER={flt}     : wall {mmm(w)}   device: mark_ms {mmm(d)}")
        del os.environ["MIEKKI_PANEL_FILTER"]
        mark_panel()
        (pw, pd), (cw, cd) = timed_pair(ix, [count_panel, count_cover])
        same = bool(np.array_equal(pcov, ccov) and np.array_equal(pcells, ccells))
        say(f"  count panel, mk_panel_count(.., 8)    : wall {mmm(pw)}   device: count_ms {mmm(pd)}   = {np.median(pd) / floor_ms:.2f} x the probe's floor")
        say(f"  count cover, 8 x mk_cover_count       : wall {mmm(cw)}   device: count_ms {mmm(cd)}   = {np.median(cd) / floor_ms:.2f} x the probe's floor")
        say(f"    8 cover passes / 1 panel pass: wall {np.median(cw) / np.median(pw):.2f}, device {np.median(cd) / np.median(pd):.2f}; the two sides' counts and cells are "
            f"{'the same' if same else 'DIFFERENT'}; cells per sample {int(pcells.min())} .. {int(pcells.max())}")
        ((w, d),) = timed_pair(ix, [count_one])
        say(f"  count panel, mk_panel_count(.., 1)    : wall {mmm(w)}   device: count_ms {mmm(d)}   (one cover pass: {np.median(cd) / SLOTS:.3f})")
        for qs in sets:
            lib.mk_qset_free(ix._h, qs)
        for d in d_seen:
            lib.mk_dev_free(ix._h, d)
        lib.mk_dev_free(ix._h, d_panel)
        ix.close()
        if not same:
            say("the panel's counts differ from the cover's: nothing above means anything")
            break
    say("(tools/panel_rate.py; host clock around calls that end in a device wait; one MI355X.)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
