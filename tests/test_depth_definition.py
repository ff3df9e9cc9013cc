"""The definition of depth (include/miekki_hip.h) on the ORACLE alone, for the two samples the GPU tests use: what
keeps those tests from passing on trivial data, that the two wordings of the median agree, and that depth's covered is the
cover's.  No code under test runs here."""
import numpy as np
import pytest

import cover_ref as cr
import depth_ref as dr
import tally_ref as tr


@pytest.fixture(scope="module")
def samples():
    made = {}

    def get(bits):
        if bits not in made:
            s = tr.Sample() if bits == 8 else tr.Sample(603, 16, 320_000, whole=())
            made[bits] = (s, dr.mult(s.o, s.queries), cr.stored(s.o))
        return made[bits]
    return get


@pytest.mark.parametrize("bits", [8, 16])
def test_sample_preconditions_and_the_two_wordings_of_the_median(samples, bits):
    s, m, fps = samples(bits)
    o = s.o
    tab = dr.table(m)
    med, total, cov = dr.profile(o, tab, fps)
    print("queries", len(s.queries), "cells", int((m > 0).sum()), "mult >= 2", int((m >= 2).sum()), "largest", int(m.max()),
          "medians", sorted(set(med.tolist())), "covered 0", int((cov == 0).sum()))
    assert 2 <= m.max() < dr.DEPTH_MAX and (m >= 2).sum() > 10_000
    assert len(set(med.tolist())) >= 5
    np.testing.assert_array_equal(med, dr.median_by_threshold(o, tab, fps))
    seen = cr.seen(o, s.queries)
    np.testing.assert_array_equal(m > 0, seen)
    np.testing.assert_array_equal(cov, cr.covered(o, seen, fps))
    assert not m[:, cr.empty_of(o)].any()
    v = dr.values(o, tab, fps)
    np.testing.assert_array_equal(total, v.sum(0).astype(np.uint64))
    assert ((med >= 1) == (cov > 0)).all() and (med.astype(np.int64) * (cov > 0) <= v.max(0)).all()


def test_the_set_taken_five_times_saturates_some_cells_and_not_others(samples):
    s, m, fps = samples(8)
    assert m.max() * 5 > dr.DEPTH_MAX                                      # (65 * 5 = 325)
    tab = dr.table(m * 5)
    assert (tab == 255).any() and ((tab > 0) & (tab < 255)).any()
    np.testing.assert_array_equal(dr.profile(s.o, tab, fps)[0], dr.median_by_threshold(s.o, tab, fps))
    # a saturated byte beside an unsaturated one in the same dword: what the marks' compare-and-swap has to keep apart
    d = tab.reshape(-1, 4)
    assert (((d == 255).any(1)) & (((d > 0) & (d < 255)).any(1))).any()
