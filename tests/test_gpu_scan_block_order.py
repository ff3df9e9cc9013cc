"""The order of scan_block_kernel's work items (SlabArgs::block_sub_fast, MIEKKI_SCAN_BLOCK_SUB_FAST = F): within a (tile,
range) runs of F consecutive 128-byte sub-tiles vary fastest, then the launch's blocks, then the 8 / F runs.  F = 8 is
sub-tile fastest, F = 1 block fastest.  The order decides which workgroups are in flight together and nothing else: every
(tile, range, block, sub-tile) is counted once and stored where it was, so every order must give the same hits.

Every case runs the block path once per order and compares it with the CPU oracle -- (genome, matches) exactly, the
intersection to 1e-6 relative, as test_gpu_scan_blocks.py's check does -- by equality with the query groups' kernel
(MIEKKI_SCAN_BLOCKS=0), and the orders with one another, hits and active counts alike.  The knobs are those of
test_gpu_scan_blocks.py.  The shapes are the smallest at which the decode of a work number can go wrong: a number of
blocks that divides nothing (3), a launch whose first block is not block 0, one block, a tile whose later sub-tiles lie
past the last genome (the early return is met at a sub-tile that is not the work number mod 8), two-byte fingerprints,
launches over a part of the ranges.

A value that is not 1, 2, 4 or 8 is handed to the launcher as it stands and refused there: the query fails with
MiekkiHipError ("... sub-tiles fastest (1, 2, 4 or 8)"), nothing is launched, and the index answers the next query.
"""
import os
import sys

import numpy as np
import pytest

import synth

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = (1, 2, 4, 8)
ENV = {"MIEKKI_SLAB_MIN_QUERIES": "1", "MIEKKI_SLAB_MIB": "1",
       "MIEKKI_SCAN_BLOCK_QUERIES": "24", "MIEKKI_SCAN_BLOCK_MIN_QUERIES": "1"}


@pytest.fixture(autouse=True)
def small_blocks_on_the_range_table_path(monkeypatch):
    for name, value in ENV.items():
        monkeypatch.setenv(name, value)


def build(k, h, fpb, genomes):
    import miekki_amd
    ix = miekki_amd.Miekki(k, h, fpb, 33, 20)
    ref = orc.OracleMiekki(k, h, fpb, 33, 20)
    for i in range(0, len(genomes), 64):
        ix.insert_sequences(genomes[i:i + 64])
        ref.insert_sequences(genomes[i:i + 64])
    return ix, ref


def queries_of(G, L, n, qlen, seed=0):
    return [synth.genome_bases(*synth.query_origin(q + seed, G, L, qlen), qlen) for q in range(n)]


def run(ix, queries, monkeypatch, blocks, order=None, nres=10, ms=2, mi=1.0):
    monkeypatch.setenv("MIEKKI_SCAN_BLOCKS", blocks)
    monkeypatch.setenv("MIEKKI_SCAN_GROUPS", "16")
    if order is None:
        monkeypatch.delenv("MIEKKI_SCAN_BLOCK_SUB_FAST", raising=False)
    else:
        monkeypatch.setenv("MIEKKI_SCAN_BLOCK_SUB_FAST", str(order))
    hits, active = ix.query(queries, nres, ms, mi)
    return [[(x.genome, x.matches, x.intersection) for x in hl] for hl in hits], np.asarray(active).copy()


def check(ix, expected, queries, monkeypatch, orders=ORDERS):
    """The block path in every order against the oracle's filtered hits `expected`, against the groups' kernel and
    against one another."""
    runs = [("groups", *run(ix, queries, monkeypatch, "0"))]
    runs += [(f, *run(ix, queries, monkeypatch, "1", f)) for f in orders]
    for q in range(len(queries)):
        w = expected[q]
        for tag, got, _ in runs:
            assert [(g, m) for g, m, _ in got[q]] == [(y[0], y[1]) for y in w], (tag, q)
            assert all(abs(x[2] - y[3]) <= 1e-6 * abs(y[3]) for x, y in zip(got[q], w)), (tag, q)
    for tag, got, active in runs[1:]:
        assert got == runs[0][1], tag
        np.testing.assert_array_equal(active, runs[0][2], err_msg=str(tag))


def oracle_hits(ref, queries, nres=10, ms=2, mi=1.0):
    want = ref.query_sequences(queries)
    return [ref.filter_results(want[q], nres, ms, mi) for q in range(len(queries))]


@pytest.fixture(scope="module")
def two_tiles():
    """1,100 genomes of 3,000 bases at one-byte fingerprints: two 1 KiB tiles, the second with one live sub-tile (76 of its
    128 genomes) and seven past the last genome; 60 queries of 400 bases
    in blocks of 24 are three blocks, the last of 12; 2^12 partitions under a 1 MiB slab are several ranges.  The oracle's
    hits are computed once."""
    G, L = 1100, 3000
    mp = pytest.MonkeyPatch()
    for name, value in ENV.items():
        mp.setenv(name, value)
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    queries = queries_of(G, L, 60, 400)
    try:
        yield ix, queries, oracle_hits(ref, queries)
    finally:
        ix.close()
        mp.undo()


def test_three_ragged_blocks_over_two_tiles(monkeypatch, two_tiles):
    """One launch of three blocks (24, 24, 12 queries): 3 F items per run of sub-tiles divide neither an XCD's round nor
    half a (tile, range), and the second tile's workgroups past the last genome leave at sub-tiles 1 to 7 in every order."""
    ix, queries, expected = two_tiles
    check(ix, expected, queries, monkeypatch)


def test_chunk_edges_inside_blocks(monkeypatch, two_tiles):
    """Chunks of 40 queries: the second launch (queries 40 to 59) begins inside block 1 and spans blocks 1 and 2 -- the
    decode adds a first block that is not 0 -- and block 1's partials are stored by two launches, each its own side."""
    monkeypatch.setenv("MIEKKI_CHUNK_QUERIES", "40")
    ix, queries, expected = two_tiles
    check(ix, expected, queries, monkeypatch)


def test_one_block(monkeypatch):
    """20 queries (one block) and 130 genomes: with one block every order is the same map; the second sub-tile holds two
    genomes, the other six none."""
    G, L = 130, 6000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        queries = queries_of(G, L, 20, 500)
        check(ix, oracle_hits(ref, queries), queries, monkeypatch)
    finally:
        ix.close()


def test_two_byte_fingerprints(monkeypatch):
    """W = 2: 600 genomes are two tiles of 512, 64 genomes per sub-tile (the second tile: one full sub-tile, one of 24
    genomes, six past the end); 31 queries are two blocks.  Block fastest and sub-tile fastest."""
    G, L = 600, 4000
    ix, ref = build(21, 12, 16, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        queries = queries_of(G, L, 31, 500)
        check(ix, oracle_hits(ref, queries), queries, monkeypatch, orders=(1, 8))
    finally:
        ix.close()


def test_staged_cold_ranges(monkeypatch):
    """A 3 MiB budget for 2^12 rows of 2 KiB (1,030 genomes), as test_gpu_scan_blocks.py has it: the cold ranges are
    staged and scanned by launches with r_begin > 0 and r_count < S, so the decode sits behind the range arithmetic.
    Block fastest."""
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "3")               # (read when the context is made)
    G, L = 1030, 3000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        queries = queries_of(G, L, 30, 400)
        check(ix, oracle_hits(ref, queries), queries, monkeypatch, orders=(1,))
    finally:
        ix.close()


def test_refused_value(monkeypatch):
    """MIEKKI_SCAN_BLOCK_SUB_FAST=3 (no divisor of a tile's eight sub-tiles) is not replaced by a default: the launcher
    refuses it, the query raises, and the same index answers in a valid order afterwards."""
    import miekki_amd
    G, L = 130, 6000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        queries = queries_of(G, L, 30, 500)
        for bad in ("3", "0", "16"):
            with pytest.raises(miekki_amd.MiekkiHipError, match="sub-tiles fastest"):
                run(ix, queries, monkeypatch, "1", bad)
        check(ix, oracle_hits(ref, queries), queries, monkeypatch, orders=(1,))
    finally:
        ix.close()
