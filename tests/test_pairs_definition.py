"""The definition of a read pair as one query (include/miekki_hip.h: mk_qset_upload_pairs), on the oracle alone through
tests/pairs_ref.py: what the pair reduces to when one mate is empty or both are the same read, the ungated sketch as the
element-wise minimum, and the sample's cases the GPU tests rest on -- mate 2 winning a partition both mates reach, equal
fingerprints whose hashes the gate answers differently, a winner the gate drops where the loser would have passed."""
import numpy as np
import pytest

import cover_ref as cv
import pairs_ref as pr
import tally_ref as tr


@pytest.fixture(scope="module", params=[8, 16])
def sample(request):
    return pr.Sample(request.param)


def test_an_empty_mate_or_the_same_mate_twice_is_the_single_read(sample):
    o = sample.o
    for a, b in sample.pairs[:40]:
        for read in (a, b):
            want = o.minhash_sketch_partition_solid_kmers(read)
            scores, active = o.query_sequence(read)
            for pair in ((read, b""), (b"", read), (read, read)):
                fp = pr.sketch(o, *pair)
                assert np.array_equal(fp, want)
                rows, act = pr.rows_of(o, [fp], sample.stored)
                assert np.array_equal(rows[0], scores) and int(act[0]) == active


def test_a_short_mate_adds_nothing(sample):
    o, k = sample.o, sample.par[0]
    a, b = sample.pairs[0]
    for L in (0, 1, k - 1, k):
        assert np.array_equal(pr.sketch(o, a, b[:L]), o.minhash_sketch_partition_solid_kmers(a))
        assert np.array_equal(pr.sketch(o, a[:L], b), o.minhash_sketch_partition_solid_kmers(b))


def test_the_ungated_sketch_is_the_minimum_of_the_mates(sample):
    o = sample.o
    for a, b in sample.pairs:
        fp, _, _ = pr.ungated(o, a, b)
        fa, fb = o.minhash_sketch_partition(a)[0], o.minhash_sketch_partition(b)[0]
        assert np.array_equal(fp, np.minimum(fa, fb))


def test_rows_from_stored_columns_are_the_oracles_rows_for_single_reads(sample):
    """pairs_ref.rows_of is query_sequences when the sketch is a single read's"""
    o = sample.o
    reads = [a for a, _ in sample.pairs[:30]]
    fps = [o.minhash_sketch_partition_solid_kmers(r) for r in reads]
    rows, active = pr.rows_of(o, fps, sample.stored)
    assert np.array_equal(rows, o.query_sequences(reads))
    assert [int(x) for x in active] == [o.query_sequence(r)[1] for r in reads]


def counts(sample):
    """(i) partitions both mates reach where mate 2 wins, (ii) equal fingerprints with different hashes whose gate answers
    differ, (iii) the winner fails the gate where the loser would pass; and the pairs that differ from their concatenation"""
    o = sample.o
    empty = cv.empty_of(o)
    n_i = n_ii = n_iii = n_cat = 0
    for a, b in sample.pairs:
        fa, ha, _ = o.minhash_sketch_partition(a)
        fb, hb, _ = o.minhash_sketch_partition(b)
        both = (fa != empty) & (fb != empty)
        n_i += int((both & (fb < fa)).sum())
        tie = np.flatnonzero(both & (fa == fb) & (ha != hb))
        n_ii += int((pr.gate(o, ha[tie]) != pr.gate(o, hb[tie])).sum())
        differ = np.flatnonzero(both & (fa != fb))
        take_b = fb[differ] < fa[differ]
        win, lose = np.where(take_b, hb[differ], ha[differ]), np.where(take_b, ha[differ], hb[differ])
        n_iii += int((~pr.gate(o, win) & pr.gate(o, lose)).sum())
        n_cat += int(not np.array_equal(pr.sketch(o, a, b), o.minhash_sketch_partition_solid_kmers(a + b)))
    return n_i, n_ii, n_iii, n_cat


def test_the_sample_holds_the_cases_the_gpu_tests_rest_on(sample):
    n_i, n_ii, n_iii, n_cat = counts(sample)
    print("bits %d: (i) %d (ii) %d (iii) %d, %d of %d pairs differ from their concatenation" % (sample.par[2], n_i, n_ii, n_iii, n_cat, len(sample.pairs)))
    assert n_i > 0 and n_iii > 0
    if sample.par[2] == 8:
        assert n_ii > 0
    assert n_cat > len(sample.pairs) // 2


def test_the_pairs_gated_sketch_is_not_the_union_of_the_mates(sample):
    o = sample.o
    empty = cv.empty_of(o)
    n = 0
    for (a, b), fp in zip(sample.pairs, sample.fps):
        ga, gb = o.minhash_sketch_partition_solid_kmers(a), o.minhash_sketch_partition_solid_kmers(b)
        n += int(not np.array_equal(fp, np.minimum(ga, gb)))
        assert ((fp == empty) | (fp == ga) | (fp == gb)).all()
    assert n > 0


def test_the_mates_as_single_reads_tally_differently(sample):
    """the profile the pairs were made for: fragments counted once, and assigned on the evidence of both mates"""
    o, thr = sample.o, sample.par[4]
    pairs = tr.tally(o, sample.rows, 10, 0.5 * thr)
    mates = tr.tally(o, o.query_sequences([m for p in sample.pairs for m in p]), 10, 0.5 * thr)
    assert not np.array_equal(pairs, mates)
    assert 0 < pairs[:, 2].sum() <= len(sample.pairs)
    # pairs that list a genome while neither mate alone lists any
    lone = [o.filter_results(r, 1, 10, 0.5 * thr) for r in o.query_sequences([m for p in sample.pairs for m in p])]
    rescued = sum(1 for i, r in enumerate(sample.rows)
                  if o.filter_results(r, 1, 10, 0.5 * thr) and not lone[2 * i] and not lone[2 * i + 1])
    print("assigned: %d pairs, %d of %d mates; %d pairs listed where neither mate is" % (int(pairs[:, 2].sum()), int(mates[:, 2].sum()), 2 * len(sample.pairs), rescued))
    assert rescued > 0
