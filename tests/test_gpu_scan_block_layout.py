"""The query-block scan's counters and row addressing (scan_block_kernel): a block's slots in LDS up to the last word of
the last one, the row home chosen once per workgroup, and a row reached by one 32 x 32-bit multiply-add onto a 64-bit
base that holds everything else.  The cases put hits into the last slot of a default block and the last word of a
sub-tile, put the hot / cold boundary on and inside a partition range, and put most rows of a matrix beyond byte 2^32.
Hits and active counts against the CPU oracle (where it is quick enough), against the query groups' kernel
(MIEKKI_SCAN_BLOCKS=0) and against the one-query-per-wave kernel (MIEKKI_SCAN_BLOCKS=0 MIEKKI_SCAN_GROUPS=0).
The knobs are those of test_gpu_scan_blocks.py.
"""
import os
import sys

import numpy as np
import pytest

import synth

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

PATHS = (("1", "16"), ("0", "16"), ("0", "0"))     # MIEKKI_SCAN_BLOCKS, MIEKKI_SCAN_GROUPS


@pytest.fixture
def small_blocks(monkeypatch):
    monkeypatch.setenv("MIEKKI_SCAN_BLOCK_QUERIES", "24")
    monkeypatch.setenv("MIEKKI_SCAN_BLOCK_MIN_QUERIES", "1")


def build(k, h, fpb, genomes):
    import miekki_amd
    ix = miekki_amd.Miekki(k, h, fpb, 33, 20)
    ref = orc.OracleMiekki(k, h, fpb, 33, 20)
    for i in range(0, len(genomes), 64):
        ix.insert_sequences(genomes[i:i + 64])
        ref.insert_sequences(genomes[i:i + 64])
    return ix, ref


def three_paths(ix, queries, monkeypatch, nres, ms, mi):
    """The hits and active counts of the three kernels; they must agree with one another."""
    runs = []
    for blocks, groups in PATHS:
        monkeypatch.setenv("MIEKKI_SCAN_BLOCKS", blocks)
        monkeypatch.setenv("MIEKKI_SCAN_GROUPS", groups)
        hits, active = ix.query(queries, nres, ms, mi)
        got = [[(x.genome, x.matches, x.intersection) for x in hl] for hl in hits]
        runs.append(((blocks, groups), got, np.asarray(active).copy()))
    for tag, got, active in runs[1:]:
        assert got == runs[0][1], tag
        np.testing.assert_array_equal(active, runs[0][2])
    return runs


def check(ix, ref, queries, monkeypatch, nres=10, ms=2, mi=1.0):
    """Every path against the oracle; returns the oracle's filtered hits per query."""
    want = ref.query_sequences(queries)
    runs = three_paths(ix, queries, monkeypatch, nres, ms, mi)
    exp = []
    for q in range(len(queries)):
        w = ref.filter_results(want[q], nres, ms, mi)
        exp.append(w)
        for tag, got, _ in runs:
            assert [(g, m) for g, m, _ in got[q]] == [(y[0], y[1]) for y in w], (tag, q)
            assert all(abs(x[2] - y[3]) <= 1e-6 * abs(y[3]) for x, y in zip(got[q], w)), (tag, q)
    return exp


def queries_of(G, L, n, qlen, seed=0):
    return [synth.genome_bases(*synth.query_origin(q + seed, G, L, qlen), qlen) for q in range(n)]


def test_last_slot_last_word_default_block(monkeypatch):
    """No block knobs: 2,437 queries of 100 bases are two full blocks of 1,216 and one of five; 260 genomes are two full
    128-byte sub-tiles and one of four bytes, where only lane 0 of a lane group has genomes and its quad is split.  The
    queries in the last slot of the full blocks (set indices 1,215 and 2,431) come from the genomes in the last byte of the
    full sub-tiles (127 and 255), query 1,216 (slot 0 of the second block) from genome 128 and query 0 from the last
    genome: the oracle has hits for exactly those, so the last slot's last word -- the last of the block's counters in LDS --
    is written and read back."""
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "1")
    monkeypatch.setenv("MIEKKI_SLAB_MIN_QUERIES", "1")
    G, L, qlen = 260, 6000, 100
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 2437, qlen)
        placed = {1215: 127, 2431: 255, 1216: 128, 0: 259}
        for q, g in placed.items():
            qs[q] = synth.genome_bases(g, 1000 + 7 * q % 3000, qlen)
        exp = check(ix, ref, qs, monkeypatch)
        for q, g in placed.items():
            assert exp[q] and exp[q][0][0] == g, (q, g)
    finally:
        ix.close()


@pytest.mark.parametrize("mib,where", [("2", "on a range boundary"), ("3", "inside a range")])
def test_home_per_workgroup(monkeypatch, small_blocks, mib, where):
    """1,030 genomes at -h 12: 2^12 rows of 2 KiB in four ranges of 1,024 (a slab of 1 MiB).  A budget of 2 MiB keeps rows
    [0, 1024) in HBM -- P_hot on the boundary of the first two ranges: every range has one home, the first in HBM, the
    others in host memory; 3 MiB keeps [0, 1536): P_hot strictly inside the second range (the budgets are
    test_gpu_scan_blocks.py's: test_staged_cold_ranges)."""
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "1")
    monkeypatch.setenv("MIEKKI_SLAB_MIN_QUERIES", "1")
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", mib)                # (read when the context is made)
    G, L = 1030, 3000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 30, 400), monkeypatch)
    finally:
        ix.close()


def test_row_offsets_past_4_gib(monkeypatch, small_blocks):
    """-h 20, 8,704 synthetic genomes of 50 kb: 2^20 rows of 9 KiB, more than half of them beyond byte 2^32 of the matrix
    -- a row offset that lost its upper half would read another row.  60 queries of 1 kb in blocks of 24 (the last one
    short) over nine tiles, the last of 512 bytes.  The three kernels give equal hits and active counts, and every
    query's top hit is the genome it was cut from.  No oracle here: it would take minutes to build this index."""
    import miekki_amd
    monkeypatch.setenv("MIEKKI_SLAB_MIN_QUERIES", "1")
    G, L, qlen = 8704, 50_000, 1000
    ix = miekki_amd.Miekki(31, 20, 8, 33, 20)
    try:
        ix.reserve(G)
        for g0 in range(0, G, 4096):
            ix.insert_synthetic(g0, min(4096, G - g0), L)
        # queries from the first, the last and scattered genomes (q * 149 mod G walks all nine tiles)
        src = [0, G - 1] + [q * 149 % G for q in range(2, 60)]
        qs = [synth.genome_bases(g, synth.query_origin(q, G, L, qlen)[1], qlen) for q, g in enumerate(src)]
        runs = three_paths(ix, qs, monkeypatch, 10, 10, 1.0)
        for q, g in enumerate(src):
            assert runs[0][1][q] and runs[0][1][q][0][0] == g, (q, g)
    finally:
        ix.close()
