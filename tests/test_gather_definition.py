"""The definition of the gather (include/miekki_hip.h) on the ORACLE alone, for the two samples the GPU tests use:
the facts the definition states, that a cap and a larger min_new give prefixes of the uncapped run at min_new 1 (which is how
the GPU tests get their other yardsticks from tests/gather_ref.py's one run per sample), and the recorded results that keep those
tests from passing on trivial data.  No code under test runs here."""
import numpy as np
import pytest

import cover_ref as cr
import depth_ref as dr
import gather_ref as gr
import winners_ref as wr

# bits: (P, G, picks at min_new 1, 10, 40, explained at 1, tie rounds at 1), recorded from this loop
RECORDED = {8: (512, 1101, 534, 256, 131, 25198, 419), 16: (512, 603, 603, 339, 300, 52417, 412)}


@pytest.fixture(scope="module")
def samples():
    return wr.samples()


@pytest.fixture(scope="module")
def runs(samples):
    return gr.runs(samples)


@pytest.mark.parametrize("bits", [8, 16])
def test_invariants_and_recorded_results(samples, runs, bits):
    w, run = samples(bits), runs(bits)
    picks, cells, explained = run.picks()
    P, G, n1, n10, n40, exp1, ties = RECORDED[bits]
    print("picks", len(picks), "explained", explained, "cells", cells, "tie rounds", run.tie_rounds, "first", picks[:3].tolist())
    assert (w.P, w.G) == (P, G)
    fresh = picks["fresh"].astype(np.int64)
    assert (np.diff(fresh) <= 0).all() and fresh.min() >= 1                # fresh never increases
    assert int(picks["genome"][0]) == int(np.argmax(w.cov)) and picks["fresh"][0] == picks["covered"][0] == w.cov.max()
    assert len(set(picks["genome"].tolist())) == len(picks) <= G           # no genome twice, at most G rounds
    np.testing.assert_array_equal(picks["covered"], w.cov[picks["genome"]])
    np.testing.assert_array_equal(picks["sketch_size"], np.asarray(w.o.sketch_size)[picks["genome"]])
    assert (picks["fresh"] <= picks["covered"]).all() and not picks["depth_sum"].any()
    assert explained == fresh.sum() == w.claimed <= cells == w.cells       # min_new 1, no cap: -W's claimed
    # the struck cells of all picks are distinct seen cells, and each pick's lie in its own column
    struck = np.concatenate([r[2] for r in run.rounds])
    assert len(np.unique(struck)) == len(struck) == explained and w.seen.reshape(-1)[struck].all()
    for g, _, cells_g, _ in run.rounds[:20]:
        np.testing.assert_array_equal(cells_g & ((1 << bits) - 1), w.fps[cells_g >> bits, g])
    assert (len(picks), int((fresh >= 10).sum()), int((fresh >= 40).sum()), explained, run.tie_rounds) == (n1, n10, n40, exp1, ties)


@pytest.mark.parametrize("bits", [8, 16])
def test_a_larger_min_new_and_a_cap_give_prefixes(samples, runs, bits):
    """runs of their own through gather_ref.gather, not through the cached run"""
    w, run = samples(bits), runs(bits)
    full = run.picks()[0]
    for m in (10, 40):
        picks, cells, explained = gr.gather(w.o, w.seen, w.fps, min_new=m)
        n = int((full["fresh"] >= m).sum())
        assert 0 < n < len(full) and cells == w.cells
        np.testing.assert_array_equal(picks, full[:n])
        np.testing.assert_array_equal(picks, run.picks(min_new=m)[0])
        assert explained == int(full["fresh"][:n].sum())
    for k in (1, 7):
        picks = gr.gather(w.o, w.seen, w.fps, max_picks=k)[0]
        np.testing.assert_array_equal(picks, full[:k])
        np.testing.assert_array_equal(picks, run.picks(max_picks=k)[0])
    both = gr.gather(w.o, w.seen, w.fps, min_new=40, max_picks=7)[0]
    np.testing.assert_array_equal(both, full[:7])


def test_depth_sums_and_reported_ids(samples, runs):
    """depth_sum is the table's bytes over the struck cells: every struck cell is seen, so at least fresh; the set taken twice
    doubles it where no byte reaches the cap.  genome is the reported id: local + base."""
    w, run = samples(8), runs(8)
    m = dr.mult(w.o, w.s.queries)
    once, twice = run.picks(table=dr.table(m))[0], run.picks(table=dr.table(2 * m))[0]
    assert 2 * m.max() < dr.DEPTH_MAX
    assert (once["depth_sum"] >= once["fresh"]).all() and (once["depth_sum"] > once["fresh"]).any()
    np.testing.assert_array_equal(twice["depth_sum"], 2 * once["depth_sum"])
    assert once["depth_sum"].sum() == m.reshape(-1)[np.concatenate([r[2] for r in run.rounds])].sum()
    capped = run.picks(table=dr.table(5 * m))[0]
    assert (capped["depth_sum"] < 5 * once["depth_sum"]).any()
    moved = run.picks(base=1000)[0]
    np.testing.assert_array_equal(moved["genome"], once["genome"] + 1000)
    direct = gr.gather(w.o, w.seen, w.fps, min_new=40, table=dr.table(m), base=7)[0]
    np.testing.assert_array_equal(direct, run.picks(min_new=40, table=dr.table(m), base=7)[0])


def test_formats():
    picks = np.zeros(2, gr.PICK)
    picks[0], picks[1] = (7, 30, 41, 500, 95), (3, 30, 30, 480, 1 << 40)
    assert gr.format_gather(picks) == b"7\t30\t41\t500\n3\t30\t30\t480\n"
    assert gr.format_gather(picks, True) == b"7\t30\t41\t500\t95\n3\t30\t30\t480\t1099511627776\n"
    assert gr.format_gather(picks[:0]) == b""
    assert gr.summary_line(620, 60, 99, 2, 10) == b"gather: 620 queries, 60 of 99 seen cells explained by 2 genomes, each at least 10 new"
