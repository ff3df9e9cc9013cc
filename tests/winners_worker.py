"""One process of tests/test_gpu_winners.py: an index of argv[1]'s genomes (a pickle: par, seqs, words), the table uploaded as it
is, mk_cover_winners under whatever MIEKKI_WIN_ROWS / MIEKKI_WIN_VALUES the environment sets; what it returns goes to argv[2]
(.npz)."""
import ctypes as C
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import miekki_amd                      # noqa: E402
from miekki_amd import lib as L        # noqa: E402


def main():
    with open(sys.argv[1], "rb") as f:
        job = pickle.load(f)
    ix = miekki_amd.Miekki(*job["par"])
    try:
        seqs = job["seqs"]
        for i in range(0, len(seqs), 64):
            ix.insert_sequences(seqs[i:i + 64])
        lib, h, G, words = ix._lib, ix._h, ix.index_size, job["words"]
        tab = C.c_void_p()
        L.check(lib.mk_dev_alloc(h, words.nbytes, C.byref(tab)))
        L.check(lib.mk_dev_upload(h, tab, words.ctypes.data, words.nbytes))
        cov, won = np.zeros(G, np.uint32), np.zeros(G, np.uint32)
        cells, claimed = C.c_uint64(0), C.c_uint64(0)
        L.check(lib.mk_cover_winners(h, tab, cov.ctypes.data, won.ctypes.data, C.byref(cells), C.byref(claimed)))
        lib.mk_dev_free(h, tab)
        np.savez(sys.argv[2], covered=cov, won=won, cells=np.uint64(cells.value), claimed=np.uint64(claimed.value))
    finally:
        ix.close()


if __name__ == "__main__":
    main()
