"""One process of tests/test_gpu_markers.py: an index of argv[1]'s genomes (a pickle: par, seqs, words, taxonomies, switches), the
table uploaded as it is, mk_taxonomy_markers of every taxonomy under the MIEKKI_MARK_ROWS the environment sets and each
setting of the job's `switches` in turn -- a dict of MIEKKI_MARK_* values, the empty one for the defaults; the library reads the
switches per call.  What the calls return goes to argv[2] (.npz): "<i>/<taxonomy>" -> uint64 [n_nodes + 1, 2],
"<i>/<taxonomy>/cells", i the setting's place in the list."""
import ctypes as C
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import miekki_amd                      # noqa: E402
from miekki_amd import lib as L        # noqa: E402

SWITCHES = ("MIEKKI_MARK_VALUES", "MIEKKI_MARK_FILTER", "MIEKKI_MARK_TOUCHED")


def main():
    with open(sys.argv[1], "rb") as f:
        job = pickle.load(f)
    ix = miekki_amd.Miekki(*job["par"])
    out = {}
    try:
        seqs = job["seqs"]
        for i in range(0, len(seqs), 64):
            ix.insert_sequences(seqs[i:i + 64])
        lib, h, G, words = ix._lib, ix._h, ix.index_size, job["words"]
        tab = C.c_void_p()
        L.check(lib.mk_dev_alloc(h, words.nbytes, C.byref(tab)))
        L.check(lib.mk_dev_upload(h, tab, words.ctypes.data, words.nbytes))
        for i, setting in enumerate(job["switches"]):
            for name in SWITCHES:
                os.environ.pop(name, None)
            os.environ.update(setting)
            for name, nodes in job["taxonomies"].items():
                lo = np.array([n[0] for n in nodes], np.uint32)
                hi = np.array([n[1] for n in nodes], np.uint32)
                t = C.c_void_p()
                L.check(lib.mk_taxonomy_create(h, lo.ctypes.data, hi.ctypes.data, len(nodes), G, C.byref(t)))
                nm, cells = np.zeros((len(nodes) + 1, 2), np.uint64), C.c_uint64(0)
                L.check(lib.mk_taxonomy_markers(h, t, tab, nm.ctypes.data, len(nm), C.byref(cells)))
                lib.mk_taxonomy_free(h, t)
                out["%d/%s" % (i, name)] = nm
                out["%d/%s/cells" % (i, name)] = np.uint64(cells.value)
        lib.mk_dev_free(h, tab)
        np.savez(sys.argv[2], **out)
    finally:
        ix.close()


if __name__ == "__main__":
    main()
