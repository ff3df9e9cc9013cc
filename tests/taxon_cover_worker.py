"""One process of tests/test_gpu_taxon_cover.py: an index of argv[1]'s genomes (a pickle: par, seqs, words, taxonomies, wides), the
table uploaded as it is, mk_taxonomy_cover of every taxonomy under the MIEKKI_TAXCOVER_ROWS the environment sets and each
MIEKKI_TAXCOVER_WIDE of the job in turn (None: unset; the library reads the switches per call); what the calls return goes to
argv[2] (.npz): "<wide>/<taxonomy>" -> uint64 [n_nodes, 2], "<wide>/<taxonomy>/cells"."""
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
    out = {}
    try:
        seqs = job["seqs"]
        for i in range(0, len(seqs), 64):
            ix.insert_sequences(seqs[i:i + 64])
        lib, h, G, words = ix._lib, ix._h, ix.index_size, job["words"]
        tab = C.c_void_p()
        L.check(lib.mk_dev_alloc(h, words.nbytes, C.byref(tab)))
        L.check(lib.mk_dev_upload(h, tab, words.ctypes.data, words.nbytes))
        for wide in job["wides"]:
            if wide is None:
                os.environ.pop("MIEKKI_TAXCOVER_WIDE", None)
            else:
                os.environ["MIEKKI_TAXCOVER_WIDE"] = str(wide)
            for name, nodes in job["taxonomies"].items():
                lo = np.array([n[0] for n in nodes], np.uint32)
                hi = np.array([n[1] for n in nodes], np.uint32)
                t = C.c_void_p()
                L.check(lib.mk_taxonomy_create(h, lo.ctypes.data, hi.ctypes.data, len(nodes), G, C.byref(t)))
                nc, cells = np.zeros((len(nodes), 2), np.uint64), C.c_uint64(0)
                L.check(lib.mk_taxonomy_cover(h, t, tab, nc.ctypes.data, C.byref(cells)))
                lib.mk_taxonomy_free(h, t)
                out["%s/%s" % (wide, name)] = nc
                out["%s/%s/cells" % (wide, name)] = np.uint64(cells.value)
        lib.mk_dev_free(h, tab)
        np.savez(sys.argv[2], **out)
    finally:
        ix.close()


if __name__ == "__main__":
    main()
