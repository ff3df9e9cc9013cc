#!/usr/bin/env python3
"""What the column gather of mk_qset_from_index costs, next to what it replaces and to the scan that follows it:
synthetic genomes (SURVEY.md 8d, 5 Mb each) at -h 20, queried 64 at a time.
  (a) sketch_ms of a set made from 64 CONSECUTIVE ids (16-byte loads)           -- the gather
  (b) sketch_ms of the same 64 genomes uploaded as sequences (mk_qset_upload)  -- what -A does for them
  (c) scan_ms of the set of (a)
  (d) sketch_ms of a set made from 64 SCATTERED ids (the byte gather)
Each figure: median [min .. max] over `reps` fresh passes (mk_qset_invalidate) after one warm-up pass, on different runs of ids.
    python tools/from_index_rate.py [genomes] [h] [fp_bits] [reps]"""
import ctypes as C
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import miekki_amd
from miekki_amd import lib as L

G = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
h = int(sys.argv[2]) if len(sys.argv) > 2 else 20
fpb = int(sys.argv[3]) if len(sys.argv) > 3 else 8
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 7
LEN = 5_000_000
lib = L.load_library()
ix = miekki_amd.Miekki(31, h, fpb, 33, 200)
ix.reserve(G + 64)
ix.insert_synthetic(0, G, LEN)
lib.mk_sync(ix._h)


def passes(qs, n, what):
    """[warm-up +] reps passes over the set -> lists of (sketch_ms, scan_ms)"""
    out = []
    hl = C.c_void_p()
    for r in range(reps + 1):
        L.check(lib.mk_qset_invalidate(ix._h, qs))
        ix.reset_stats()
        if what == "sketch":
            act = np.zeros(n, np.uint32)
            L.check(lib.mk_qset_active(ix._h, qs, act.ctypes.data))
        else:
            L.check(lib.mk_qset_run_list(ix._h, qs, 10, 10, 100.0, C.byref(hl)))
            lib.mk_hitlist_free(hl)
        L.check(lib.mk_sync(ix._h))
        st = ix.stats()
        if r:
            out.append((st["sketch_ms"], st["scan_ms"]))
    return out


def fmt(v):
    return f"{statistics.median(v):.3f} ms [{min(v):.3f} .. {max(v):.3f}]"


rng = np.random.default_rng(1)
gather, scan, upload, scattered = [], [], [], []
for start in (0, 64 * 100 + 5, G // 2 + 17, G - 64):                # aligned, unaligned, the last run
    start = max(0, min(start, G - 64))
    ids = np.arange(start, start + 64, dtype=np.uint32)
    qs = C.c_void_p()
    L.check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, 64, C.byref(qs)))
    gather += [s for s, _ in passes(qs, 64, "sketch")]
    scan += [c for _, c in passes(qs, 64, "run")]
    lib.mk_qset_free(ix._h, qs)
for _ in range(2):
    ids = np.sort(rng.choice(G, 64, replace=False)).astype(np.uint32)[::-1].copy()
    qs = C.c_void_p()
    L.check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, 64, C.byref(qs)))
    scattered += [s for s, _ in passes(qs, 64, "sketch")]
    lib.mk_qset_free(ix._h, qs)
# (b): the same genomes' sequences, as -A would read them from their files
start = max(0, min(64 * 100 + 5, G - 64))
buf = np.empty(64 * LEN, np.uint8)
L.check(lib.mk_probe_synth_genomes(ix._h, start, 64, LEN, buf.ctypes.data))
ptrs = (C.c_void_p * 64)(*[buf.ctypes.data + i * LEN for i in range(64)])
lens = (C.c_uint64 * 64)(*[LEN] * 64)
qs = C.c_void_p()
L.check(lib.mk_qset_upload(ix._h, ptrs, lens, 64, C.byref(qs)))
upload = [s for s, _ in passes(qs, 64, "sketch")]
lib.mk_qset_free(ix._h, qs)
print(f"{G} genomes, -h {h}, {fpb}-bit fingerprints, sets of 64 whole-genome queries, {reps} passes per set after one warm-up")
print(f"(a) gather of 64 consecutive ids (4 runs of ids): {fmt(gather)}")
print(f"(b) sketch of the same 64 genomes from their sequences: {fmt(upload)}")
print(f"(c) scan of the set of (a): {fmt(scan)}")
print(f"(d) byte gather of 64 scattered ids (2 sets): {fmt(scattered)}")
ix.close()
