"""The definition of a read with base qualities as one query (include/miekki_hip.h: mk_qset_upload_reads), on the oracle alone
through tests/reads_ref.py: what it reduces to without a bad base and with one, a read that is all bad, and the edge list the
GPU tests rest on."""
import numpy as np
import pytest

import cover_ref as cv
import pairs_ref as pr
import reads_ref as rr

K = rr.K


@pytest.fixture(scope="module", params=[8, 16])
def sample(request):
    return pr.Sample(request.param)


def test_segments_are_the_maximal_runs_of_good_bases():
    s = b"ACGTACGTAC"
    assert rr.segments(s, b"IIIIIIIIII", 20) == [s]
    assert rr.segments(s, b"#IIII#II##", 20) == [b"CGTA", b"GT"]
    assert rr.segments(s, b"##########", 20) == []
    assert rr.segments(s, b"##########", 0) == [s]
    assert rr.segments(s, bytes([52]) * 5 + bytes([53]) * 5, 20) == [s[5:]]     # 33 + 20 = 53 is good
    assert rr.segments(b"", b"", 20) == []


def test_min_qual_0_is_the_plain_read_and_the_plain_pair(sample):
    o = sample.o
    for (a, qa), (b, qb) in rr.sample_reads(sample.seqs, 30):
        fp = rr.sketch(o, 0, (a, qa))
        assert np.array_equal(fp, o.minhash_sketch_partition_solid_kmers(a))
        rows, act = pr.rows_of(o, [fp], sample.stored)
        scores, active = o.query_sequence(a)
        assert np.array_equal(rows[0], scores) and int(act[0]) == active
        assert np.array_equal(rr.sketch(o, 0, (a, qa), (b, qb)), pr.sketch(o, a, b))


def test_one_bad_base_at_c_is_the_pair_of_what_lies_before_and_after(sample):
    o = sample.o
    n = 0
    for a, _ in sample.pairs[:25]:
        for c in (0, 1, K, len(a) // 2, len(a) - K - 1, len(a) - 1):
            fp = rr.sketch(o, rr.MIN_QUAL, (a, rr.mask(len(a), [c])))
            assert np.array_equal(fp, pr.sketch(o, a[:c], a[c + 1:]))
            n += int(not np.array_equal(fp, o.minhash_sketch_partition_solid_kmers(a)))
    assert n > 25


def test_a_read_that_is_all_bad_has_no_active_partition(sample):
    o = sample.o
    a, b = sample.pairs[0]
    empty = cv.empty_of(o)
    assert (rr.sketch(o, rr.MIN_QUAL, (a, rr.mask(len(a), range(len(a))))) == empty).all()
    assert (rr.sketch(o, 93, (a, rr.mask(len(a))), (b, rr.mask(len(b)))) == empty).all()
    # no stretch of k + 1 good bases: the same
    assert (rr.sketch(o, rr.MIN_QUAL, (a, rr.mask(len(a), range(K, len(a), K + 1)))) == empty).all()


def test_the_edge_list_is_not_trivial(sample):
    o = sample.o
    edges = rr.edge_reads(sample.seqs)
    rows, active = rr.rows(o, rr.MIN_QUAL, [((s, q),) for _, s, q in edges], sample.stored)
    plain = o.query_sequences([s for _, s, _ in edges])
    by = {what: i for i, (what, _, _) in enumerate(edges)}
    differ = sum(1 for i in range(len(edges)) if not np.array_equal(rows[i], plain[i]))
    print("bits %d: %d of %d edge rows differ from the uncut read's, largest score %d" % (sample.par[2], differ, len(edges), rows.max()))
    assert differ > len(edges) // 2
    assert rows[by["nk 4065 bad 100"]].max() > 50 and rows[by["nk 257 bad 129,162"]].max() > 10
    assert rows[by["indexed repeats with cuts"]].max() > 5 and rows[by["repeats with cuts"]].max() == 0
    assert active[by["every base bad"]] == 0 and active[by["length %d" % K]] == 0 and active.max() > 300
    assert np.array_equal(rows[by["none bad"]], plain[by["none bad"]])
    # a segment of k bases has no k-mer, one of k + 1 has one
    assert active[by["two bad bases %d apart at the head" % (K + 1)]] == active[by["two bad bases %d apart at the head" % K]]
    # seeds: where the N stands in a later segment matters as it does in the first
    assert not np.array_equal(rows[by["N at 0 of the segment at 81"]], rows[by["N at %d of the segment at 81" % (K - 1)]])
    pairs = rr.edge_pairs(sample.seqs)
    prow, pact = rr.rows(o, rr.MIN_QUAL, [(a, b) for _, a, b in pairs], sample.stored)
    assert prow.max() > 50 and pact[[w for w, _, _ in pairs].index("both empty")] == 0
    assert len({r.tobytes() for r in prow}) > len(pairs) // 2
