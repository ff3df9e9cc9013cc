#!/usr/bin/env python3
"""What mk_index_select costs, next to the only route there was before it and to the device's stream rate: a synthetic
index (mk_index_append_synthetic), and wall time around the call + mk_sync for four lists --
  identity                       (nothing moves: the call returns after its checks)
  every genome but each 64th     (ascending with gaps: the span path, 16-byte loads through LDS)
  reversal                       (descending: the byte gather, neighbouring sources)
  a seeded random permutation    (the byte gather, scattered sources)
each on a freshly permuted index of the same size (a select shrinks or reorders the index it is given; the lists after
the first run on the result of the one before, which for a synthetic index is the same work).
Yardsticks printed beside them: the matrix bytes, mk_probe_stream_read's rate and bytes / rate, and the export-then-import
route (mk_index_export_genomes to the host, mk_index_import_columns back).  The route is timed on a SAMPLE -- 512 genomes
exported, 1/256 of the rows imported -- and scaled to the whole list, because at 100,000 genomes it moves 105 GB each way.
    python tools/select_rate.py [genomes] [h] [fp_bits] [genome length]"""
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import miekki_amd
from miekki_amd import lib as L

G = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
h = int(sys.argv[2]) if len(sys.argv) > 2 else 20
fpb = int(sys.argv[3]) if len(sys.argv) > 3 else 8
LEN = int(sys.argv[4]) if len(sys.argv) > 4 else 100_000
W, P = fpb // 8, 1 << h
lib = L.load_library()
ix = miekki_amd.Miekki(31, h, fpb, 33, 200)
ix.reserve(G)
t0 = time.perf_counter()
ix.insert_synthetic(0, G, LEN)
L.check(lib.mk_sync(ix._h))
print(f"{G} synthetic genomes of {LEN} bases, -h {h}, {fpb}-bit fingerprints: built in {time.perf_counter() - t0:.1f} s")
matrix = P * G * W
gbps, nbytes = C.c_double(), C.c_uint64()
L.check(lib.mk_probe_stream_read(ix._h, 3, C.byref(gbps), C.byref(nbytes)))
print(f"matrix: {matrix / 1e9:.2f} GB ({P} rows x {G * W} bytes); mk_probe_stream_read: {gbps.value:.0f} GB/s over {nbytes.value / 1e9:.2f} GB"
      f" -> one read of the matrix {matrix / gbps.value / 1e6:.1f} ms, one read + one write {2 * matrix / gbps.value / 1e6:.1f} ms")


def timed_select(name, ids):
    ids = np.ascontiguousarray(ids, np.uint32)
    t = time.perf_counter()
    L.check(lib.mk_index_select(ix._h, ids.ctypes.data, len(ids)))
    L.check(lib.mk_sync(ix._h))
    dt = time.perf_counter() - t
    moved = 2 * P * len(ids) * W
    print(f"{name}: n = {len(ids)}: {dt * 1e3:.1f} ms ({moved / dt / 1e9:.0f} GB/s of rows read + written)")
    return dt


rng = np.random.default_rng(1)
n = ix.index_size
timed_select("identity", np.arange(n))
timed_select("seeded random permutation", rng.permutation(n))
timed_select("reversal", np.arange(n)[::-1])
timed_select("every genome but each 64th", np.array([g for g in range(n) if g % 64 != 63]))
n = ix.index_size
# the route there was before: columns of the list to the host 64 genomes at a time, the rows back in partition ranges
m = min(512, n)
ids = np.ascontiguousarray(rng.permutation(n)[:m], np.uint32)
buf = np.empty(P * m * W, np.uint8)
t = time.perf_counter()
L.check(lib.mk_index_export_genomes(ix._h, ids.ctypes.data, m, buf.ctypes.data))
t_exp = (time.perf_counter() - t) * n / m
rows = max(1, P // 256)
buf = np.empty(rows * n * W, np.uint8)
L.check(lib.mk_index_export_columns(ix._h, 0, rows, buf.ctypes.data))
t = time.perf_counter()
L.check(lib.mk_index_import_columns(ix._h, 0, rows, buf.ctypes.data))
L.check(lib.mk_sync(ix._h))
t_imp = (time.perf_counter() - t) * P / rows
print(f"export-then-import route for a list of {n} (scaled from {m} genomes exported, {rows} of {P} rows imported): "
      f"export {t_exp:.1f} s + import {t_imp:.1f} s = {t_exp + t_imp:.1f} s, and {2 * P * n * W / 1e9:.1f} GB over PCIe")
ix.close()
