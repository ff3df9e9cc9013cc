"""mk_query_list / mk_qset_run_list (filter_results for any nresults): the ABI surface, and the checker the GPU tests of
the lists rely on -- mk_filter_candidates with nresults = the number of candidates must be the oracle's filter_results
with nresults = the index size, ties included.  No GPU needed."""
import ctypes
import os
import re

import numpy as np

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mk_query_list", "mk_qset_run_list", "mk_hitlist_offsets", "mk_hitlist_hits", "mk_hitlist_free"]


def test_header_declares_and_library_exports_the_list_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    lib = ctypes.CDLL(L.library_path())
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), f"{s} is not declared in include/miekki_hip.h"
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in L.SIGNATURES
    assert re.search(r"#define\s+MK_ALL_RESULTS\s+0xffffffffu", text)
    assert L.ALL_RESULTS == 0xffffffff
    assert "typedef struct mk_hitlist mk_hitlist;" in text


def test_abi_version_and_structs_did_not_move():
    assert L.load_library().mk_abi_version() == 5
    assert ctypes.sizeof(L.Stats) == 16 * 8 and ctypes.sizeof(L.Hit) == 24 and ctypes.sizeof(L.Params) == 32


def test_python_surface():
    import inspect
    from miekki_amd import Miekki
    sig = inspect.signature(Miekki.query_list)
    assert [p for p in sig.parameters][1:] == ["seqs", "nresults", "min_score", "min_intersection"]
    assert sig.parameters["nresults"].default is None and sig.parameters["min_score"].default == 10
    assert inspect.signature(Miekki.query_file).parameters["nresults"].default == 10
    assert inspect.signature(Miekki.query).parameters["nresults"].default == 10


def test_filter_candidates_over_all_candidates_is_the_oracle_with_nresults_index_size(golden_dir):
    """The yardstick of tests/test_gpu_query_list.py: no eviction ever happens, and the order of equal intersections is
    what libstdc++'s push_heap sequence followed by sort_heap leaves -- on both sides."""
    from oracle import oracle as orc
    lib = L.load_library()
    gold = np.load(os.path.join(golden_dir, "filter_ties.npz"))
    compared = 0
    for c in range(int(gold["n"])):
        G, _, ms = (int(x) for x in gold[f"c{c}_par"])
        mi = float(gold[f"c{c}_mi"])
        ss, gs, sc = gold[f"c{c}_ss"], gold[f"c{c}_gs"], gold[f"c{c}_sc"]
        o = orc.OracleMiekki(21, 8, 8, 32, 10)
        o.poke_sizes(ss, gs)
        want = o.filter_results(sc, G, ms, mi)
        cand = (L.Hit * max(G, 1))()
        n = 0
        for g in range(G):
            if sc[g] < ms:
                continue
            jac = float(sc[g]) / float(ss[g])
            inter = jac * float(gs[g])
            if inter < mi:
                continue
            cand[n] = L.Hit(g, int(sc[g]), jac, inter)
            n += 1
        out = (L.Hit * max(n, 1))()
        m = lib.mk_filter_candidates(cand, n, n, out)
        assert m == n == len(want), c
        assert [(out[i].genome, out[i].matches, out[i].jaccard, out[i].intersection) for i in range(m)] == want, c
        compared += m
    assert compared > 500
