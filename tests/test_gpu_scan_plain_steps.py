"""The plain kernel's compare steps (scan_kernel.hpp: list_step) against the CPU oracle: the full, the windowed and the
ragged step are one function that differs in which entries it keeps, so the score rows of queries whose entry counts sit
on every edge of that function must equal the oracle's exactly.

A query's entry count is its number of active partitions.  The plain kernel walks it in chunks of 255 entries (what the
packed 8-bit counters hold; 65,535 at 16 bits) and a chunk in steps of eight, so the counts wanted are: a multiple of
eight (no ragged step), one more (a ragged step of one entry), seven more (of seven), a count in 248..255 (one chunk, its
last full step and tail), one in 256..263 (a second chunk that is only a ragged step) and one above 510 (three chunks).
The lengths below were found with the oracle on the CPU; the test asserts the counts ON THE ORACLE before it looks at
the device, so a change of the generator shows up there and not as a weaker test.

Miekki.query_sequences reaches scan_kernel<.., WINDOW = false> with the matrix in HBM, and <.., WINDOW = true> -- one
launch per window of rows, later windows adding to the rows -- under MIEKKI_HBM_MATRIX_MIB=1, which leaves 1,024
(512) of the 4,096 rows in HBM.  It lays score rows out in whole tiles (16-byte stores); the same queries as a prepared
set give rows of pitch G through mk_qset_scores, which 130 and 1,100 genomes make too narrow or unaligned for 16-byte
stores: the scalar store and add paths.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import synth

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

K, H = 21, 12
OFFSET = 100
# (bits per fingerprint, genomes, genome length, query lengths): query i is cut from genome 13 i + 3 at OFFSET
CASES = {
    "G130": (8, 130, 6000, (29, 30, 31, 37, 300, 299, 295, 310, 583, 621)),     # less than a tile, ragged
    "G1100": (8, 1100, 3000, (29, 30, 31, 37, 300, 299, 295, 310, 583, 621)),   # two tiles, the second ragged
    "W2_G600": (16, 600, 3000, (28, 29, 30, 36, 282, 285, 286, 292, 560, 586)),  # two tiles of 512 genomes, the second ragged
}


def queries_of(seqs, lengths):
    qs = [seqs[13 * i + 3][OFFSET:OFFSET + n] for i, n in enumerate(lengths)]
    return qs + [b"", seqs[0][:K - 1]]                            # no entries at all: rows of zeros


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    """genomes, queries, the oracle's rows and active counts: made once per case"""
    fpb, G, L, lengths = CASES[request.param]
    seqs = [synth.genome_bases(g, 0, L) for g in range(G)]
    ref = orc.OracleMiekki(K, H, fpb, 33, 20)
    ref.insert_sequences(seqs)
    qs = queries_of(seqs, lengths)
    want = ref.query_sequences(qs)
    want.setflags(write=False)
    active = [ref.query_sequence(q)[1] for q in qs]
    return fpb, seqs, qs, want, active


def test_oracle_counts_cover_the_step_forms(case):
    fpb, _, _, _, active = case
    assert {0, 1, 7} <= {a % 8 for a in active if a}, active
    assert any(248 <= a <= 255 for a in active), active
    assert any(256 <= a <= 263 for a in active), active
    assert any(a > 510 for a in active), active
    assert active[-2:] == [0, 0], active


def device_rows(fpb, seqs, qs):
    """(query_sequences' rows, mk_qset_scores' rows of pitch G, the device's active counts, scan launches that
    query_sequences made) of a fresh context"""
    import miekki_amd
    import torch
    from miekki_amd import lib as L
    G = len(seqs)
    ix = miekki_amd.Miekki(K, H, fpb, 33, 20)
    lib = L.load_library()
    qset = C.c_void_p()
    try:
        for i in range(0, G, 256):
            ix.insert_sequences(seqs[i:i + 256])
        before = ix.stats()["scan_launches"]
        rows = ix.query_sequences(qs)
        launches = ix.stats()["scan_launches"] - before
        ptrs, lens = L.seq_arrays(qs)
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, len(qs), C.byref(qset)))
        d = torch.full((len(qs) * G,), -1, dtype=torch.int32, device="cuda")
        L.check(lib.mk_qset_scores(ix._h, qset, 0, len(qs), d.data_ptr()))
        L.check(lib.mk_sync(ix._h))
        act = np.zeros(len(qs), np.uint32)
        L.check(lib.mk_qset_active(ix._h, qset, act.ctypes.data))
        return rows, d.cpu().numpy().view(np.uint32).reshape(len(qs), G), act, launches
    finally:
        if qset:
            lib.mk_qset_free(ix._h, qset)
        ix.close()


@pytest.mark.parametrize("budget_mib", [None, "1"], ids=["hbm", "windowed"])
def test_score_rows_equal_the_oracle(case, monkeypatch, budget_mib):
    fpb, seqs, qs, want, active = case
    if budget_mib is None:
        monkeypatch.delenv("MIEKKI_HBM_MATRIX_MIB", raising=False)
    else:
        monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", budget_mib)   # (read when the context is made)
    rows, set_rows, act, launches = device_rows(fpb, seqs, qs)
    # all rows in HBM: the set is one launch of the unwindowed kernel; with cold rows: a launch per window of rows, the
    # hot part and at least one staged cold window, each adding to the rows of the one before
    assert launches == 1 if budget_mib is None else launches >= 2, launches
    assert [int(a) for a in act] == active
    np.testing.assert_array_equal(rows, want)
    np.testing.assert_array_equal(set_rows, want)
