"""The query-block scan (scan_block_kernel) at the edges of its lane mapping and of its packed counters: a lane group per
128-byte row piece, 16 bytes per lane, a lane whose bytes begin at or beyond the last genome neither loading nor adding,
a block of 1,280 queries in all of a CU's LDS.  The shapes are the smallest at which a mapping with more bytes per lane or
wider LDS adds could go wrong as well (both were tried and not kept; the cases stay for the next attempt):
collections that end on, one past and one short of every 16-byte piece and 32-byte pair of pieces up to the last quad of
the last sub-tile; a (query, range) whose counters end at 255 (300 at two-byte fingerprints) on both sides of a word
boundary inside an aligned 8 bytes, beside a counter of 0; the last slot of a full default block; packets of three pairs
that meet dead lanes; rows staged from a cold range.

Every case compares hits and active counts of the block path with the CPU oracle -- (genome, matches) exactly, the
intersection to 1e-6 relative, as test_gpu_scan_blocks.py's check does -- and by equality with the query groups' kernel
(MIEKKI_SCAN_BLOCKS=0) and the one-query-per-wave kernel (MIEKKI_SCAN_BLOCKS=0 MIEKKI_SCAN_GROUPS=0).  The knobs are
those of test_gpu_scan_blocks.py; the steered sequences are scan_limits.py's.
"""
import os
import sys

import numpy as np
import pytest

import scan_limits as sl
import synth

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

PATHS = (("1", "16"), ("0", "16"), ("0", "0"))     # MIEKKI_SCAN_BLOCKS, MIEKKI_SCAN_GROUPS


@pytest.fixture(autouse=True)
def range_table_path(monkeypatch):
    monkeypatch.setenv("MIEKKI_SLAB_MIN_QUERIES", "1")
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "1")


@pytest.fixture
def small_blocks(monkeypatch):
    monkeypatch.setenv("MIEKKI_SCAN_BLOCK_QUERIES", "24")
    monkeypatch.setenv("MIEKKI_SCAN_BLOCK_MIN_QUERIES", "1")


def build(k, h, fpb, genomes, bloom=33):
    import miekki_amd
    ix = miekki_amd.Miekki(k, h, fpb, bloom, 20)
    ref = orc.OracleMiekki(k, h, fpb, bloom, 20)
    for i in range(0, len(genomes), 64):
        ix.insert_sequences(genomes[i:i + 64])
        ref.insert_sequences(genomes[i:i + 64])
    return ix, ref


def check(ix, ref, queries, monkeypatch, nres=10, ms=2, mi=1.0):
    """The three kernels against the oracle and against one another; returns the oracle's filtered hits per query."""
    want = ref.query_sequences(queries)
    runs = []
    for blocks, groups in PATHS:
        monkeypatch.setenv("MIEKKI_SCAN_BLOCKS", blocks)
        monkeypatch.setenv("MIEKKI_SCAN_GROUPS", groups)
        hits, active = ix.query(queries, nres, ms, mi)
        got = [[(x.genome, x.matches, x.intersection) for x in hl] for hl in hits]
        runs.append(((blocks, groups), got, np.asarray(active).copy()))
    exp = []
    for q in range(len(queries)):
        w = ref.filter_results(want[q], nres, ms, mi)
        exp.append(w)
        for tag, got, _ in runs:
            assert [(g, m) for g, m, _ in got[q]] == [(y[0], y[1]) for y in w], (tag, q)
            assert all(abs(x[2] - y[3]) <= 1e-6 * abs(y[3]) for x, y in zip(got[q], w)), (tag, q)
    for tag, got, active in runs[1:]:
        assert got == runs[0][1], tag
        np.testing.assert_array_equal(active, runs[0][2])
    return exp


def queries_of(G, L, n, qlen, seed=0):
    return [synth.genome_bases(*synth.query_origin(q + seed, G, L, qlen), qlen) for q in range(n)]


HALVES = [(8, G) for G in (16, 17, 31, 32, 33, 48, 112, 127, 128, 129, 144)] + [(16, G) for G in (8, 9, 24, 56, 64, 65, 72)]


@pytest.mark.parametrize("fpb,G", HALVES)
def test_halves_of_a_lane(monkeypatch, small_blocks, fpb, G):
    """Collections that end on, one past and one short of a lane's 16 bytes, of 32 bytes and of a 128-byte sub-tile: the
    lane after the last live one dead, a lane with one live byte (half-word), the last quad of the last sub-tile.  30
    queries in blocks of 24; one is cut from the last genome and, for every boundary between two 16-byte pieces, one from
    the genome before it and one from the genome after it: each must come back as its query's top hit."""
    per_half = 16 // (fpb // 8)
    L, qlen = 6000, 500
    ix, ref = build(21, 12, fpb, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 30, qlen)
        src = [G - 1] + [g for j in range(1, (G - 1) // per_half + 1) for g in (per_half * j - 1, per_half * j)]
        assert len(src) <= 30
        at = [24 + i if i < 6 else i - 6 for i in range(len(src))]    # (the first six in the second, short block)
        for q, g in zip(at, src):
            qs[q] = synth.genome_bases(g, 1000 + 37 * q, qlen)
        exp = check(ix, ref, qs, monkeypatch)
        for q, g in zip(at, src):
            assert exp[q] and exp[q][0][0] == g, (q, g)
    finally:
        ix.close()


@pytest.mark.parametrize("fpb,want", [(8, 255), (16, 300)])
def test_counters_full_on_both_sides_of_a_word_boundary(monkeypatch, small_blocks, fpb, want):
    """A steered query (scan_limits.steered) with exactly `want` entries in partition range 1 of 4 -- 255 is all a byte
    counter holds -- against 40 genomes: two copies of the steered sequence itself, which match every entry (a mismatch
    counter of 0), and 38 short genomes that match none, so that their counters of that range end at `want`.  Genomes
    3 and 4 (at 16 bits 1 and 2) are the top counter of a low word and the bottom counter of the high word of one aligned
    8 bytes; the copies sit in the bottom counter of the following 8 bytes (genome 8 / 4) and of a high word in the next
    lane's bytes (genome 20 / 10), each right above a full counter: a carry out of a word or of a pair of words would make
    them 1.  The oracle alone is asked first: `want` entries in the range, nothing matched by the fillers, everything by
    the copies."""
    W, k, S, r, G = fpb // 8, 21, 4, 1, 40
    bare = orc.OracleMiekki(k, 12, fpb, sl.BLOOM_LOG2, sl.THRESHOLD)
    seq = sl.steered(bare, S, r, want, 1000 * want + r)
    pool = [synth.genome_bases(50_000 + i, 0, k + 40 + i % 30) for i in range(96)]
    pre = orc.OracleMiekki(k, 12, fpb, sl.BLOOM_LOG2, sl.THRESHOLD)
    pre.insert_sequences([seq] + pool)
    none = [pool[int(i)] for i in np.flatnonzero(pre.query_sequences([seq])[0][1:] == 0)]
    copies = (8 // W, 20 // W)
    assert len(none) >= G - len(copies)
    fill = iter(none)
    genomes = [seq if g in copies else next(fill) for g in range(G)]
    ix, ref = build(k, 12, fpb, genomes, bloom=sl.BLOOM_LOG2)
    try:
        qs = [genomes[7 * q % G][:55] for q in range(29)] + [seq]      # (the steered query in either block, between short ones)
        qs[5] = seq
        assert sl.per_range(ref, S, seq)[r] == want
        row = ref.query_sequences([seq])[0]
        entries = len(sl.gated_partitions(ref, seq))
        assert len(seq) - k <= S * sl.HOST_MEAN or W == 2      # (the host keeps S = 4: it doubles S by the k-mers of one-byte sets only)
        assert [int(row[g]) for g in copies] == [entries, entries]
        assert not any(int(row[g]) for g in range(G) if g not in copies)
        exp = check(ix, ref, qs, monkeypatch, ms=1, mi=0.0)
        for q in (5, 29):
            assert sorted((y[0], y[1]) for y in exp[q]) == [(g, entries) for g in copies], q
    finally:
        ix.close()


def test_last_slot_of_a_full_block(monkeypatch):
    """No block knobs: 2,565 queries of 100 bases are two full blocks of 1,280 -- all of a CU's LDS -- and one of five; 260
    genomes are two full 128-byte sub-tiles and one of four bytes.  Queries 1,279 and 2,559 (the last slot of the full
    blocks) are cut from genomes 127 and 255 (the last byte of the full sub-tiles), query 1,280 (slot 0 of the second
    block) from genome 128 and query 0 from the last genome, in the ragged sub-tile."""
    G, L, qlen = 260, 6000, 100
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 2565, qlen)
        placed = {1279: 127, 1280: 128, 2559: 255, 0: 259}
        for q, g in placed.items():
            qs[q] = synth.genome_bases(g, 1000 + 7 * q % 3000, qlen)
        exp = check(ix, ref, qs, monkeypatch)
        for q, g in placed.items():
            assert exp[q] and exp[q][0][0] == g, (q, g)
    finally:
        ix.close()


@pytest.mark.parametrize("fpb,G", [(8, 40), (8, 144), (16, 40)])
def test_many_pairs_meet_dead_halves(monkeypatch, small_blocks, fpb, G):
    """test_gpu_scan_blocks.py's 60 + 12 copies -- partitions that eight and twelve queries of a block of 24 want: packets of
    three pairs, more packets than a step has in flight -- against collections that end half way into a lane's 16 bytes
    and an odd number of 16-byte pieces into the sub-tile (40 genomes: 40 of 48 bytes; at 16 bits 80 of 96) and whose
    second sub-tile is a single live lane per group (144)."""
    L = 40_000
    genomes = [synth.genome_bases(g, 0, L) for g in range(G - 1)] + [synth.tandem_rich(7, L, 0.5)]
    ix, ref = build(21, 12, fpb, genomes)
    try:
        base = queries_of(G, L, 3, 700)
        qs = [base[i % 3] for i in range(60)] + [genomes[-1][1000:1800]] * 12
        check(ix, ref, qs, monkeypatch, ms=10, mi=10.0)
    finally:
        ix.close()


def test_cold_range_rows(monkeypatch, small_blocks):
    """1,030 genomes at -h 12 under a budget of 2 MiB: rows [0, 1024) stay in HBM, the other three ranges are staged from
    host memory (test_gpu_scan_block_layout.py: test_home_per_workgroup); the second tile is six bytes of one lane."""
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "2")                # (read when the context is made)
    G, L = 1030, 3000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 30, 400)
        qs[29] = synth.genome_bases(G - 1, 500, 400)
        exp = check(ix, ref, qs, monkeypatch)
        assert exp[29] and exp[29][0][0] == G - 1
    finally:
        ix.close()
