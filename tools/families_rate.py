#!/usr/bin/env python3
"""mk_index_families next to the route that gave the same answer before it existed -- every genome's list of hits above the
thresholds (mk_qset_from_index + mk_qset_run_list, MK_LIST_CANDIDATES) and a union-find on the host -- on the same device
in the same run:
  (a) `species` x 64 strains (mk_index_append_synthetic_strains), families of 64        default 20,000 genomes
  (b) ONE species of `dense` strains: every genome lists every other                     default 8,192 genomes
-k 31 -h 17, one-byte fingerprints, genomes of 50,000 bases (partial sketches: genome_size does not wrap), -s 2000, i.e.
min_score 10 and min_intersection 1,000: unrelated genomes share ~70 of ~48,000 fingerprints by chance (an estimated
intersection of ~70), a strain at 1,000 substitutions per million keeps ~97 % of its 31-mers, so every strain lists its
species' strain 0 with an estimate in the tens of thousands.  The labels of both routes are checked against the
generator's own species ids.  Host memory: ru_maxrss after each route (the family route runs first: the figure only grows).
    python tools/families_rate.py [genomes_a] [genomes_b]"""
import ctypes as C
import os
import resource
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import miekki_amd
from miekki_amd import lib as L
from miekki_amd.index import _HIT_DTYPE

GA = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
GB = int(sys.argv[2]) if len(sys.argv) > 2 else 8_192
LEN, RATE_PPM, H, THRESHOLD = 50_000, 1000, 17, 2000
lib = L.load_library()


def rss_mib():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def list_route(ix):
    """(labels, seconds in the lists, seconds in the host union-find, pairs)"""
    G = ix.index_size
    per = max(64, min(4096, (2 << 30) // (3 * ix.number_minimizer * ix.W)) // 64 * 64)
    t0 = time.perf_counter()
    qa, ga = [], []
    for i in range(0, G, per):
        ids = np.arange(i, min(i + per, G), dtype=np.uint32)
        qs, hl = C.c_void_p(), C.c_void_p()
        L.check(lib.mk_qset_from_index(ix._h, ids.ctypes.data, len(ids), C.byref(qs)))
        try:
            L.check(lib.mk_qset_run_list(ix._h, qs, L.LIST_CANDIDATES, 10, 0.5 * THRESHOLD, C.byref(hl)))
            off = np.ctypeslib.as_array(lib.mk_hitlist_offsets(hl), (len(ids) + 1,)).astype(np.int64)
            rec = np.zeros(int(off[-1]), _HIT_DTYPE)
            if len(rec):
                C.memmove(rec.ctypes.data, lib.mk_hitlist_hits(hl), rec.nbytes)
            lib.mk_hitlist_free(hl)
        finally:
            lib.mk_qset_free(ix._h, qs)
        qa.append(np.repeat(ids, np.diff(off)))
        ga.append(rec["genome"].copy())
    a, b = np.concatenate(qa), np.concatenate(ga)
    t1 = time.perf_counter()
    lab = np.arange(G, dtype=np.uint32)                              # min-label propagation with pointer jumping
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return lab, t1 - t0, time.perf_counter() - t1, len(a)


def measure(tag, G, strains):
    ix = miekki_amd.Miekki(31, H, 8, 33, THRESHOLD)
    try:
        ix.reserve(G + 64)
        ix.insert_synthetic_strains(0, G, LEN, strains, RATE_PPM)
        L.check(lib.mk_sync(ix._h))
        want = (np.arange(G, dtype=np.uint32) // strains) * strains      # the species' strain 0
        ix.families()                                                    # warm-up: buffers, code objects
        ix.reset_stats()
        t0 = time.perf_counter()
        fam = ix.families()
        t_fam = time.perf_counter() - t0
        st = ix.stats()
        rss_fam = rss_mib()
        lab, t_list, t_union, pairs = list_route(ix)
        rss_list = rss_mib()
        ok = np.array_equal(fam, want) and np.array_equal(lab, want)
        print(f"({tag}) {G} genomes, {strains} strains per species: labels {'equal the species ids on both routes' if ok else 'DIFFER from the species ids'}")
        print(f"    mk_index_families: {t_fam:.3f} s (sketch {st['sketch_ms']:.1f} ms, scan {st['scan_ms']:.1f} ms, link {st['filter_ms']:.1f} ms), host peak {rss_fam:.0f} MiB")
        print(f"    lists + host union-find: {t_list:.3f} s + {t_union:.3f} s for {pairs} pairs, host peak {rss_list:.0f} MiB")
        return ok
    finally:
        ix.close()


print(f"-k 31 -h {H}, one-byte fingerprints, {LEN}-base genomes, {RATE_PPM} substitutions per million, min_score 10, min_intersection {0.5 * THRESHOLD:.0f}")
good = measure("a", GA, 64)
good = measure("b", GB, GB) and good
sys.exit(0 if good else 1)
