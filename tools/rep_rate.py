#!/usr/bin/env python3
"""mk_index_representatives next to mk_index_families on the same index in the same run, alternating: the scans are the same
launches, the difference is the bitmap rows (G / 8 bytes written per query, where the link sink writes nothing) and the
sequential resolve per set.  The index is the strain collection of tools/families_rate.py (a): `genomes` genomes in species
of 64 strains (mk_index_append_synthetic_strains), -k 31 -h 17, one-byte fingerprints, 50,000-base genomes, -s 2000, i.e.
min_score 10 and min_intersection 1,000.  Every strain lists its species' strain 0 and no other species, so both answers
are the species' strain 0 for every genome: checked.  Wall clock around calls that end in a synchronise; sketch_ms /
scan_ms / filter_ms from mk_stats (device events).
    python tools/rep_rate.py [genomes] [repeats]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import miekki_amd
from miekki_amd import lib as L

G = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LEN, RATE_PPM, H, THRESHOLD, STRAINS = 50_000, 1000, 17, 2000, 64
lib = L.load_library()


def timed(ix, call):
    ix.reset_stats()
    t0 = time.perf_counter()
    out = call()
    t = time.perf_counter() - t0
    st = ix.stats()
    return out, t, st


ix = miekki_amd.Miekki(31, H, 8, 33, THRESHOLD)
try:
    ix.reserve(G + 64)
    ix.insert_synthetic_strains(0, G, LEN, STRAINS, RATE_PPM)
    L.check(lib.mk_sync(ix._h))
    want = (np.arange(G, dtype=np.uint32) // STRAINS) * STRAINS
    ix.families(); ix.representatives()                                 # warm-up: buffers, code objects
    print(f"{G} genomes in species of {STRAINS}, -k 31 -h {H}, one-byte fingerprints, {LEN}-base genomes, min_score 10, min_intersection {0.5 * THRESHOLD:.0f}")
    rows = {"families": [], "representatives": []}
    ok = True
    for r in range(REPEATS):
        for name, call in (("families", ix.families), ("representatives", ix.representatives)):
            out, t, st = timed(ix, call)
            ok = ok and np.array_equal(out, want)
            rows[name].append((t, st["sketch_ms"], st["scan_ms"], st["filter_ms"]))
            print(f"  run {r} {name:16s} wall {t * 1e3:8.1f} ms   sketch {st['sketch_ms']:7.1f}  scan {st['scan_ms']:7.1f}  filter {st['filter_ms']:7.1f} ms")
    med = {k: np.median(np.array(v), axis=0) for k, v in rows.items()}
    for k, m in med.items():
        print(f"median {k:16s} wall {m[0] * 1e3:8.1f} ms   sketch {m[1]:7.1f}  scan {m[2]:7.1f}  filter {m[3]:7.1f} ms")
    print(f"representatives / families: wall {med['representatives'][0] / med['families'][0]:.2f} x")
    print("answers: " + ("both equal the species' strain 0 for every genome" if ok else "DIFFER from the species' strain 0"))
finally:
    ix.close()
sys.exit(0 if ok else 1)
