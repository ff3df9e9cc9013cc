"""The premise of mk_qset_from_index and `miekki -X`, proved with the oracle alone (no GPU): after insert_sequences, the
stored column of genome g IS what query_sequence computes for g's sequence before it scans -- the sketch is the same
function on both sides (Miekki.cpp:281, 320), the stored value of partition p is the query's first[p] (228-239, 291), and
the Bloom gate (135-146) passes every active partition of an inserted genome (295-299, 121-131; no cell returns to zero).
Plus the ABI surface of the three calls."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mk_qset_from_index", "mk_qset_from_columns", "mk_index_export_genomes_device"]


@pytest.mark.parametrize("name", ["messy", "rnd0", "rnd3", "w16", "h16z"])
def test_gated_sketch_of_an_indexed_genome_is_its_column(name):
    from oracle import oracle as orc
    case = synth.CASES[name]()
    seqs = case.genome_sequences()
    o = orc.OracleMiekki(case.k, case.h, case.fp_bits, case.b, case.threshold)
    o.insert_sequences(seqs)
    cols = o.columns()
    W, empty = o.W, (1 << case.fp_bits) - 1
    ss = o.sketch_size
    for g, s in enumerate(seqs):
        col = cols[:, g].astype(np.uint16) if W == 1 else (cols[:, 2 * g].astype(np.uint16) << 8) | cols[:, 2 * g + 1]
        fp = o.minhash_sketch_partition_solid_kmers(s)
        np.testing.assert_array_equal(fp, col, err_msg=f"{name} genome {g}")
        assert int((fp != empty).sum()) == int(ss[g]) == o.query_sequence(s)[1], (name, g)


def test_header_declares_and_library_exports_the_calls():
    from miekki_amd import lib as L
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    lib = ctypes.CDLL(L.library_path())
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in include/miekki_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in L.SIGNATURES
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)
    assert L.load_library().mk_abi_version() == 5
    assert ctypes.sizeof(L.Stats) == 16 * 8 and ctypes.sizeof(L.Hit) == 24 and ctypes.sizeof(L.Params) == 32


def test_python_surface():
    from miekki_amd import Miekki
    sig = inspect.signature(Miekki.query_indexed)
    assert [p for p in sig.parameters][1:] == ["ids", "nresults", "min_score", "min_intersection"]
    assert sig.parameters["ids"].default is None and sig.parameters["nresults"].default == 10
    assert sig.parameters["min_score"].default == 10 and sig.parameters["min_intersection"].default is None
    sig = inspect.signature(Miekki.query_index_file)
    assert [p for p in sig.parameters][1:] == ["out", "names", "nresults"]
    assert sig.parameters["names"].default is None and sig.parameters["nresults"].default == 10
