"""One process of tests/test_gpu_depth.py: an index of argv[1]'s genomes (a pickle: par, seqs, table), the table uploaded as it
is, mk_depth_profile under whatever MIEKKI_DEPTH_ROWS the environment sets; what it returns goes to argv[2] (.npz)."""
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
        lib, h, G, table = ix._lib, ix._h, ix.index_size, job["table"]
        tab = C.c_void_p()
        L.check(lib.mk_dev_alloc(h, table.nbytes, C.byref(tab)))
        L.check(lib.mk_dev_upload(h, tab, table.ctypes.data, table.nbytes))
        depth = (L.Depth * G)()
        cells, saturated = C.c_uint64(0), C.c_uint64(0)
        L.check(lib.mk_depth_profile(h, tab, depth, C.byref(cells), C.byref(saturated)))
        lib.mk_dev_free(h, tab)
        np.savez(sys.argv[2], median=np.array([d.median for d in depth], np.uint32), sum=np.array([d.sum for d in depth], np.uint64),
                 covered=np.array([d.covered for d in depth], np.uint32), cells=np.uint64(cells.value), saturated=np.uint64(saturated.value))
    finally:
        ix.close()


if __name__ == "__main__":
    main()
