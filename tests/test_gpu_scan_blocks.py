"""The query-block scan (scan_block_kernel): the range-table path of the slab schedule for sets of at least a block of
queries, where a workgroup counts a block of queries in LDS against a 128-byte sub-tile of the rows, from a list grouped
by partition.  Hits and active counts against the CPU oracle, against the query groups' kernel (MIEKKI_SCAN_BLOCKS=0)
and against the one-query-per-wave kernel (MIEKKI_SCAN_BLOCKS=0 MIEKKI_SCAN_GROUPS=0) on the same inputs.

Small cases need knobs to reach that path: MIEKKI_SLAB_MIN_QUERIES lifts the small-set cut by count, MIEKKI_SLAB_MIB
shrinks the slab so that even 2^12 partitions are cut into several ranges, MIEKKI_SCAN_BLOCK_QUERIES makes a block small
enough that a few dozen queries are several, MIEKKI_SCAN_BLOCK_MIN_QUERIES lets a set that small take the path.
"""
import os
import sys

import numpy as np
import pytest

import synth

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def range_table_path(monkeypatch):
    monkeypatch.setenv("MIEKKI_SLAB_MIN_QUERIES", "1")
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "1")


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


def check(ix, ref, queries, monkeypatch, nres=10, ms=10, mi=10.0):
    want = ref.query_sequences(queries)
    runs = []
    for blocks, groups in (("1", "16"), ("0", "16"), ("0", "0")):
        monkeypatch.setenv("MIEKKI_SCAN_BLOCKS", blocks)
        monkeypatch.setenv("MIEKKI_SCAN_GROUPS", groups)
        hits, active = ix.query(queries, nres, ms, mi)
        got = [[(x.genome, x.matches, x.intersection) for x in hl] for hl in hits]
        runs.append(((blocks, groups), got, np.asarray(active).copy()))
    for q in range(len(queries)):
        w = ref.filter_results(want[q], nres, ms, mi)
        exp = [(y[0], y[1]) for y in w]
        for tag, got, _ in runs:
            assert [(g, m) for g, m, _ in got[q]] == exp, (tag, q)
            assert all(abs(x[2] - y[3]) <= 1e-6 * abs(y[3]) for x, y in zip(got[q], w)), (tag, q)
    for tag, got, active in runs[1:]:
        assert got == runs[0][1], tag
        np.testing.assert_array_equal(active, runs[0][2])


def queries_of(G, L, n, qlen, seed=0):
    return [synth.genome_bases(*synth.query_origin(q + seed, G, L, qlen), qlen) for q in range(n)]


def test_below_one_sub_tile_ragged_blocks(monkeypatch, small_blocks):
    """12 genomes (less than a sub-tile), 25 queries (a full block of 24 and a block of one), then an empty query, one
    shorter than k and one from no genome."""
    G, L = 12, 60_000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 25, 600)
        qs += [b"", b"ACGTACGT", synth.genome_bases(999, 0, 900)]
        check(ix, ref, qs, monkeypatch)
    finally:
        ix.close()


def test_ragged_sub_tile(monkeypatch, small_blocks):
    """130 genomes: the second 128-byte sub-tile is partly past the last genome, the other six lie past it."""
    G, L = 130, 6000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 30, 500), monkeypatch, ms=2, mi=1.0)
    finally:
        ix.close()


def test_ragged_tile(monkeypatch, small_blocks):
    """1,100 genomes: the second 1 KiB tile is partly past the last genome."""
    G, L = 1100, 3000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 29, 400), monkeypatch, ms=2, mi=1.0)
    finally:
        ix.close()


def test_many_pairs_per_row(monkeypatch, small_blocks):
    """60 queries that are copies of three sequences, and twelve copies of a tandem-rich one: partitions that eight and twelve
    queries of a block of 24 want -- more pairs than a packet holds, than a step has in flight, and than eight."""
    G, L = 40, 40_000
    genomes = [synth.genome_bases(g, 0, L) for g in range(G - 1)] + [synth.tandem_rich(7, L, 0.5)]
    ix, ref = build(21, 12, 8, genomes)
    try:
        base = queries_of(G, L, 3, 700)
        qs = [base[i % 3] for i in range(60)] + [genomes[-1][1000:1800]] * 12
        check(ix, ref, qs, monkeypatch)
    finally:
        ix.close()


def test_queries_missing_ranges(monkeypatch, small_blocks):
    """30-base queries (a few k-mers) leave most (query, range) pairs without entries: zero partials are stored."""
    G, L = 30, 20_000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 40, 30) + queries_of(G, L, 4, 800, seed=50)
        check(ix, ref, qs, monkeypatch, ms=1, mi=0.0)
    finally:
        ix.close()


def test_two_byte_fingerprints(monkeypatch, small_blocks):
    """W = 2: 16-bit counters, 512 genomes per tile and 64 per sub-tile (600 genomes: two tiles)."""
    G, L = 600, 4000
    ix, ref = build(21, 12, 16, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 31, 500), monkeypatch, ms=2, mi=1.0)
    finally:
        ix.close()


def test_chunk_edges_inside_blocks(monkeypatch, small_blocks):
    """Chunks of 17 queries against blocks of 24: every chunk boundary but the set's ends falls inside a block."""
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "17")
    G, L = 20, 30_000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 60, 500), monkeypatch)
    finally:
        ix.close()


def test_staged_cold_ranges(monkeypatch, small_blocks):
    """A 3 MiB budget for 2^12 rows of 2 KiB (1,030 genomes): rows [0, 1536) stay in HBM -- of four ranges the first whole,
    the second across the boundary, the others in host memory -- so the launches walk ranges r_begin ... by r_count."""
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "3")               # (read when the context is made)
    G, L = 1030, 3000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 30, 400), monkeypatch, ms=2, mi=1.0)
    finally:
        ix.close()


def test_default_block_and_threshold(monkeypatch):
    """No block knobs: 1,300 queries of 120 bases against 140 genomes are two blocks of the default size, the second
    short, in a set just over the default threshold."""
    G, L = 140, 6000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 1300, 120), monkeypatch, ms=2, mi=1.0)
    finally:
        ix.close()
