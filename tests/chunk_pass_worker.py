"""One process of tests/test_gpu_chunk_pass.py: the four entry points that run the chunk pass, over a small strain index, with
whatever MIEKKI_CHUNK_QUERIES the environment sets; everything they return goes to argv[1] (.npz)."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import miekki_amd                      # noqa: E402
import synth                           # noqa: E402
from miekki_amd import lib as L        # noqa: E402
from miekki_amd.index import _HIT_DTYPE  # noqa: E402

G, ST, PPM, GL = 48, 16, 3000, 100_000      # three species of sixteen strains
NRES, CAP, MS, MI = 10, 64, 10, 100.0


def cut(n, qlen, seed):
    rng = np.random.default_rng(seed)
    return [synth.strain_device(int(g), ST, PPM, int(off), qlen)
            for g, off in zip(rng.integers(0, G, n), rng.integers(0, GL - qlen, n))]


def run_set(ix, name, seqs, out):
    lib, h, nq = ix._lib, ix._h, len(seqs)
    before = ix.stats()

    def dev(nbytes):
        p = C.c_void_p()
        L.check(lib.mk_dev_alloc(h, nbytes, C.byref(p)))
        return p

    def down(p, arr):
        L.check(lib.mk_dev_download(h, arr.ctypes.data, p, arr.nbytes))
        return arr

    ptrs, lens = L.seq_arrays(seqs)
    qs = C.c_void_p()
    L.check(lib.mk_qset_upload(h, ptrs, lens, nq, C.byref(qs)))
    d_count, d_cand, d_forest = dev(4 * nq), dev(nq * CAP * _HIT_DTYPE.itemsize), dev(4 * (G + nq))
    try:
        # mk_qset_run: counts and the candidates they count (the slots behind them are nobody's)
        L.check(lib.mk_qset_run(h, qs, NRES, MS, MI, CAP, d_count, d_cand))
        L.check(lib.mk_sync(h))
        count = down(d_count, np.zeros(nq, np.uint32))
        cand = down(d_cand, np.zeros((nq, CAP), _HIT_DTYPE))
        assert count.max() <= CAP
        out[name + "_run_count"] = count
        out[name + "_run_cand"] = np.concatenate([cand[q, :count[q]] for q in range(nq)])
        # mk_qset_run_list: offsets and hits, every genome above the thresholds
        hl = C.c_void_p()
        L.check(lib.mk_qset_run_list(h, qs, L.ALL_RESULTS, MS, MI, C.byref(hl)))
        off = np.ctypeslib.as_array(lib.mk_hitlist_offsets(hl), (nq + 1,)).copy()
        hits = np.zeros(int(off[nq]), _HIT_DTYPE)
        if len(hits):
            C.memmove(hits.ctypes.data, lib.mk_hitlist_hits(hl), hits.nbytes)
        lib.mk_hitlist_free(hl)
        out[name + "_list_off"], out[name + "_list_hits"] = off, hits
        # mk_qset_run_link + mk_link_labels: query q stands for id G + q
        ids = np.arange(G, G + nq, dtype=np.uint32)
        L.check(lib.mk_link_reset(h, d_forest, G + nq))
        L.check(lib.mk_qset_run_link(h, qs, ids.ctypes.data, MS, MI, d_forest, G + nq))
        labels = np.full(G + nq, 0xffffffff, np.uint32)
        L.check(lib.mk_link_labels(h, d_forest, G + nq, labels.ctypes.data))
        out[name + "_labels"] = labels
    finally:
        lib.mk_qset_free(h, qs)
        for p in (d_count, d_cand, d_forest):
            lib.mk_dev_free(h, p)
    # mk_query: the hits it reports
    got, act = ix.query(seqs, NRES, MS, MI)
    out[name + "_query_n"] = np.array([len(r) for r in got], np.uint32)
    out[name + "_query_hits"] = np.array([tuple(x) for r in got for x in r], _HIT_DTYPE)
    out[name + "_query_act"] = act
    after = ix.stats()
    out[name + "_launches"] = np.array([after[k] - before[k] for k in ("scan_launches", "scan_slab_launches")], np.int64)


def main():
    ix = miekki_amd.Miekki(31, 14, 8, 33, 200)
    out = {}
    try:
        ix.insert_synthetic_strains(0, G, GL, ST, PPM)
        short = cut(40, 1000, 5)
        run_set(ix, "short", short, out)                         # range table and query groups (the test's environment)
        run_set(ix, "long", cut(36, 4500, 6), out)               # more k-mers than the short path takes: the plain schedule
        run_set(ix, "mixed", short[:20] + cut(1, 9000, 7) + short[20:], out)   # a shell over a slab part and a plain part
    finally:
        ix.close()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
