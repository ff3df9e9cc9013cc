"""The query-group scan (scan_group_kernel): the range-table path of the slab schedule, where a wave carries a group of
queries and walks their merged entry list.  Hits and scores against the CPU oracle and against the one-query-per-wave
kernel (MIEKKI_SCAN_GROUPS=0) on the same inputs.

Small cases need knobs to reach that path: MIEKKI_SLAB_MIN_QUERIES lifts the small-set cut by count, MIEKKI_SLAB_MIB
shrinks the slab so that even 2^12 partitions are cut into several ranges, MIEKKI_GROUP_WINDOW makes the windows small
enough that a range holds several.
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


def build(k, h, fpb, genomes):
    import miekki_amd
    ix = miekki_amd.Miekki(k, h, fpb, 33, 20)
    ref = orc.OracleMiekki(k, h, fpb, 33, 20)
    for i in range(0, len(genomes), 64):
        ix.insert_sequences(genomes[i:i + 64])
        ref.insert_sequences(genomes[i:i + 64])
    return ix, ref


def check(ix, ref, queries, monkeypatch, nres=10, ms=10, mi=10.0, windows=("10", "6")):
    want = ref.query_sequences(queries)
    runs = []
    for groups in ("16", "0"):
        for wnd in windows if groups != "0" else windows[:1]:
            monkeypatch.setenv("MIEKKI_SCAN_GROUPS", groups)
            monkeypatch.setenv("MIEKKI_GROUP_WINDOW", wnd)
            hits, active = ix.query(queries, nres, ms, mi)
            got = [[(x.genome, x.matches, x.intersection) for x in hl] for hl in hits]
            runs.append(((groups, wnd), got, np.asarray(active).copy()))
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


def test_below_one_tile_ragged_groups(monkeypatch):
    """12 genomes (less than a tile), 17 queries (a full group of sixteen and one of one), an empty query, one
    shorter than k and one from no genome."""
    G, L = 12, 60_000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 14, 600)
        qs += [b"", b"ACGTACGT", synth.genome_bases(999, 0, 900)]
        check(ix, ref, qs, monkeypatch)
    finally:
        ix.close()


def test_single_group_ragged_tile(monkeypatch):
    """1,100 genomes: the second tile is partly past the last genome; five queries: one group, short."""
    G, L = 1100, 3000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 5, 400), monkeypatch, ms=2, mi=1.0)
    finally:
        ix.close()


def test_two_byte_fingerprints(monkeypatch):
    """W = 2: 16-bit counters, 512 genomes per tile (600 genomes: two tiles)."""
    G, L = 600, 4000
    ix, ref = build(21, 12, 16, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        check(ix, ref, queries_of(G, L, 21, 500), monkeypatch, ms=2, mi=1.0)
    finally:
        ix.close()


def test_repeat_rich_same_partitions(monkeypatch):
    """Many queries on the same partitions: copies of a few sequences and of a tandem-rich one, so that groups hold
    long runs of the same partitions and every slot of a group meets the same rows."""
    G, L = 40, 40_000
    genomes = [synth.genome_bases(g, 0, L) for g in range(G - 1)] + [synth.tandem_rich(7, L, 0.5)]
    ix, ref = build(21, 12, 8, genomes)
    try:
        base = queries_of(G, L, 3, 700)
        qs = [base[i % 3] for i in range(20)] + [genomes[-1][1000:1800]] * 5
        check(ix, ref, qs, monkeypatch)
    finally:
        ix.close()


def test_queries_missing_ranges(monkeypatch):
    """Short queries (a few k-mers) leave most (query, range) pairs without entries: zero partials."""
    G, L = 30, 20_000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 19, 30) + queries_of(G, L, 4, 800, seed=50)
        check(ix, ref, qs, monkeypatch, ms=1, mi=0.0)
    finally:
        ix.close()


def test_mixed_set(monkeypatch):
    """Short queries next to long ones (more k-mers than the short path takes): the short part keeps the slab schedule."""
    G, L = 20, 30_000
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 9, 500) + [synth.genome_bases(3, 0, 9000)] + queries_of(G, L, 6, 700, seed=20)
        check(ix, ref, qs, monkeypatch, windows=("10",))
    finally:
        ix.close()
