#!/usr/bin/env python3
"""mk_index_hierarchy with four levels next to the only route to the same labels before it existed -- four calls of
mk_index_families, one per level -- on the same index in the same process, alternating.  The index is the strain collection
of tools/families_rate.py (a): `genomes` genomes in species of 64 strains (mk_index_append_synthetic_strains), -k 31 -h 17,
one-byte fingerprints, 50,000-base genomes.  The two routes' labels must be identical, level by level: checked in the run.
Also: the link walk of ONE level through the level loop against mk_index_families' link walk (what the loop costs when it
has nothing to do), and the fold alone over forests filled by raw passes.  Wall clock around calls that end in a
synchronise; sketch_ms / scan_ms / filter_ms from mk_stats (device events; filter = the link walks, not the fold).
    python tools/hierarchy_rate.py [genomes] [repeats]"""
import ctypes as C
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
LEVELS = [(10, 1000.0), (10, 20000.0), (30000, 20000.0), (40000, 47000.0)]
lib = L.load_library()


def timed(ix, call):
    ix.reset_stats()
    t0 = time.perf_counter()
    out = call()
    t = time.perf_counter() - t0
    st = ix.stats()
    return out, (t * 1e3, st["sketch_ms"], st["scan_ms"], st["filter_ms"])


def four_calls(ix):
    return np.stack([ix.families(*lv) for lv in LEVELS])


def fold_alone(ix):
    """ms of mk_link_fold_levels over forests that one raw pass over the index has filled (wall clock between two synchronises)"""
    n = len(LEVELS)
    lv = (L.Level * n)(*[L.Level(s, 0, mi) for s, mi in LEVELS])
    forests = C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, 4 * n * G, C.byref(forests)))
    try:
        for l in range(n):
            L.check(lib.mk_link_reset(ix._h, C.c_void_p(forests.value + 4 * l * G), G))
        for g0 in range(0, G, 4096):
            ids = np.arange(g0, min(g0 + 4096, G), dtype=np.uint32)
            qs = C.c_void_p()
            L.check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, len(ids), C.byref(qs)))
            try:
                L.check(lib.mk_qset_run_link_levels(ix._h, qs, ids.ctypes.data, lv, n, forests, G))
            finally:
                lib.mk_qset_free(ix._h, qs)
        L.check(lib.mk_sync(ix._h))
        t0 = time.perf_counter()
        L.check(lib.mk_link_fold_levels(ix._h, forests, G, n))
        L.check(lib.mk_sync(ix._h))
        first = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        L.check(lib.mk_link_fold_levels(ix._h, forests, G, n))
        L.check(lib.mk_sync(ix._h))
        return first, (time.perf_counter() - t0) * 1e3
    finally:
        lib.mk_dev_free(ix._h, forests)


ix = miekki_amd.Miekki(31, H, 8, 33, THRESHOLD)
try:
    ix.reserve(G + 64)
    ix.insert_synthetic_strains(0, G, LEN, STRAINS, RATE_PPM)
    L.check(lib.mk_sync(ix._h))
    ix.families(*LEVELS[0]); ix.hierarchy(LEVELS); ix.hierarchy(LEVELS[:1]); fold_alone(ix)     # warm-up: buffers, code objects
    print(f"{G} genomes in species of {STRAINS}, -k 31 -h {H}, one-byte fingerprints, {LEN}-base genomes")
    print("levels (min_score, min_intersection): " + ", ".join(f"({s}, {mi:.0f})" for s, mi in LEVELS))
    routes = (("hierarchy, 4 levels", lambda: ix.hierarchy(LEVELS)), ("families x 4", lambda: four_calls(ix)),
              ("hierarchy, 1 level", lambda: ix.hierarchy(LEVELS[:1])), ("families x 1", lambda: ix.families(*LEVELS[0])[None, :]))
    rows = {name: [] for name, _ in routes}
    outs, same = {}, True
    for r in range(REPEATS):
        for name, call in routes:
            outs[name], row = timed(ix, call)
            rows[name].append(row)
            print(f"  run {r} {name:20s} wall {row[0]:8.1f} ms   sketch {row[1]:7.1f}  scan {row[2]:7.1f}  link {row[3]:7.2f} ms")
        same = same and outs["hierarchy, 4 levels"].tobytes() == outs["families x 4"].tobytes() and \
            outs["hierarchy, 1 level"].tobytes() == outs["families x 1"].tobytes()
    med = {k: np.median(np.array(v), axis=0) for k, v in rows.items()}
    for k, m in med.items():
        print(f"median {k:20s} wall {m[0]:8.1f} ms   sketch {m[1]:7.1f}  scan {m[2]:7.1f}  link {m[3]:7.2f} ms")
    folds = np.array([fold_alone(ix) for _ in range(REPEATS)])
    print(f"fold of 4 forests alone (3 merge launches over {G} ids), median of {REPEATS}: {np.median(folds[:, 0]):.3f} ms; a second fold {np.median(folds[:, 1]):.3f} ms")
    print(f"hierarchy(4 levels) / one families call: wall {med['hierarchy, 4 levels'][0] / med['families x 1'][0]:.2f} x;  / four families calls: {med['hierarchy, 4 levels'][0] / med['families x 4'][0]:.2f} x")
    print(f"link walk, 1 level through the level loop / mk_index_families' link walk: {med['hierarchy, 1 level'][3] / med['families x 1'][3]:.2f} x")
    fam = outs["hierarchy, 4 levels"]
    print("families per level: " + " / ".join(str(int((fam[l] == np.arange(G)).sum())) for l in range(len(LEVELS))))
    print("labels: " + ("the two routes are identical, level by level" if same else "the two routes DIFFER"))
finally:
    ix.close()
sys.exit(0 if same else 1)
