#!/usr/bin/env python3
"""What mk_index_extend costs, next to a 2-D copy of the same bytes and to the device's stream rate: a synthetic index
(mk_index_append_synthetic) reserved for what is to come, joined with
  one a twentieth of its size    (a day's new genomes: short spans at an odd offset in every row)
  one of its own size            (two halves built in parallel)
and wall time around each call + mk_sync.  Beside each: the bytes the columns take (read + written), hipMemcpy2D of the same
width and height between two device buffers of the two matrices' pitches (what ensure_capacity's re-layout uses, and what
extend_place_kernel could be replaced by), and mk_probe_stream_read's rate with bytes / rate.  The call also copies the sizes
and folds the Bloom filter; both are printed as what is left of the call after the rows.
    python tools/extend_rate.py [genomes] [h] [fp_bits] [genome length]
Not measured yet: the output belongs in profiles/extend_rate.txt."""
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import miekki_amd
from miekki_amd import lib as L

G = int(sys.argv[1]) if len(sys.argv) > 1 else 50_000
h = int(sys.argv[2]) if len(sys.argv) > 2 else 20
fpb = int(sys.argv[3]) if len(sys.argv) > 3 else 8
LEN = int(sys.argv[4]) if len(sys.argv) > 4 else 100_000
W, P = fpb // 8, 1 << h
lib = L.load_library()
hiprt = C.CDLL("libamdhip64.so")
hiprt.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
hiprt.hipMemcpy2D.restype = C.c_int


def pitch(genomes):
    return (genomes * W + 1023) // 1024 * 1024


def synthetic(first, n, room):
    ix = miekki_amd.Miekki(31, h, fpb, 33, 200)
    ix.reserve(room)
    t0 = time.perf_counter()
    ix.insert_synthetic(first, n, LEN)
    L.check(lib.mk_sync(ix._h))
    print(f"{n} synthetic genomes of {LEN} bases, -h {h}, {fpb}-bit fingerprints: built in {time.perf_counter() - t0:.1f} s")
    return ix


def copy_2d(ix, n_dst, n_src):
    """hipMemcpy2D of n_src * W bytes x P rows from a buffer of src's pitch to offset n_dst * W of one of dst's pitch"""
    ld_d, ld_s = pitch(n_dst + n_src), pitch(n_src)
    d, s = C.c_void_p(), C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, P * ld_d, C.byref(d)))
    L.check(lib.mk_dev_alloc(ix._h, P * ld_s, C.byref(s)))
    try:
        best = None
        for _ in range(3):
            L.check(lib.mk_sync(ix._h))
            t = time.perf_counter()
            rc = hiprt.hipMemcpy2D(d.value + n_dst * W, ld_d, s, ld_s, n_src * W, P, 3)     # 3: device to device
            dt = time.perf_counter() - t
            if rc != 0:
                raise RuntimeError(f"hipMemcpy2D failed: {rc}")
            best = dt if best is None else min(best, dt)
    finally:
        lib.mk_dev_free(ix._h, d); lib.mk_dev_free(ix._h, s)
    return best


dst = synthetic(0, G, 2 * G + G // 20)
gbps, nbytes = C.c_double(), C.c_uint64()
L.check(lib.mk_probe_stream_read(dst._h, 3, C.byref(gbps), C.byref(nbytes)))
print(f"mk_probe_stream_read: {gbps.value:.0f} GB/s over {nbytes.value / 1e9:.2f} GB")
for label, n in (("a twentieth", max(1, G // 20)), ("its own size", G)):
    src = synthetic(10_000_000, n, n)
    n_dst = dst.index_size
    t = time.perf_counter()
    dst.extend(src)
    L.check(lib.mk_sync(dst._h))
    dt = time.perf_counter() - t
    src.close()
    moved = 2 * P * n * W
    t2d = copy_2d(dst, n_dst, n)
    print(f"joined with {label} ({n} genomes behind {n_dst}, destination offset {n_dst * W % 16} modulo 16): mk_index_extend {dt * 1e3:.1f} ms "
          f"({moved / dt / 1e9:.0f} GB/s of rows read + written over the whole call); hipMemcpy2D of the same bytes {t2d * 1e3:.1f} ms "
          f"({moved / t2d / 1e9:.0f} GB/s); at the stream rate {moved / gbps.value / 1e6:.1f} ms")
dst.close()
