"""The definition of a panel (include/miekki_hip.h) on the ORACLE alone, for the two samples the GPU tests use: a panel of one
sample is the cover, a slot's plane of the expected table is that sample's cover table, and the union over the slots is the
cover of all the queries.  What keeps the GPU tests from passing on trivial data.  No code under test runs here."""
import numpy as np
import pytest

import cover_ref as cr
import panel_ref as pr
import tally_ref as tr


@pytest.fixture(scope="module")
def samples():
    made = {}

    def get(bits):
        if bits not in made:
            s = tr.Sample() if bits == 8 else tr.Sample(603, 16, 320_000, whole=())
            dealt = pr.deal(s)
            made[bits] = (s, dealt, pr.seen_per_sample(s.o, dealt), cr.stored(s.o))
        return made[bits]
    return get


@pytest.mark.parametrize("bits", [8, 16])
def test_a_panel_of_one_sample_is_the_cover(samples, bits):
    s, dealt, seens, fps = samples(bits)
    o = s.o
    one = seens[4]
    tab = pr.table([one])
    assert set(np.unique(tab).tolist()) == {0, 1}
    np.testing.assert_array_equal(pr.plane(tab, 0, o.P, bits), one)
    cov, cells = pr.count_table(o, tab, 1, fps)
    np.testing.assert_array_equal(cov[0], cr.covered(o, one, fps))
    assert cells[0] == one.sum() and cov[0].max() > 0
    # as packed bits it is the cover table itself
    np.testing.assert_array_equal(cr.unpack(cr.pack(pr.plane(tab, 0, o.P, bits)), o.P, bits), one)


@pytest.mark.parametrize("bits", [8, 16])
def test_planes_are_the_samples_and_their_union_is_the_whole(samples, bits):
    s, dealt, seens, fps = samples(bits)
    o = s.o
    sizes = [len(q) for q in dealt]
    assert len(dealt) == pr.SLOTS and 0 in sizes and 1 in sizes and len(set(sizes)) >= 7
    tab = pr.table(seens)
    cov, cells = pr.count_table(o, tab, pr.SLOTS, fps)
    print("bits", bits, "sizes", sizes, "cells", cells.tolist(), "distinct bytes", len(np.unique(tab)), "largest covered", cov.max(1).tolist())
    for slot in range(pr.SLOTS):
        np.testing.assert_array_equal(pr.plane(tab, slot, o.P, bits), cr.seen(o, dealt[slot]))
    np.testing.assert_array_equal(cov, pr.covered(o, seens, fps))
    np.testing.assert_array_equal(cells, pr.cells(seens))
    everything = [q for sample in dealt for q in sample]
    np.testing.assert_array_equal(tab.reshape(o.P, -1) != 0, cr.seen(o, everything))
    # not trivial: samples differ, bytes carry several bits at once, `empty` is never seen, the empty sample covers nothing
    assert len(np.unique(tab)) > 16 and not tab.reshape(o.P, -1)[:, cr.empty_of(o)].any()
    assert not cov[2].any() and cells[2] == 0 and all(cov[i].any() for i in range(pr.SLOTS) if i != 2)
    assert len({cov[i].tobytes() for i in range(pr.SLOTS)}) == pr.SLOTS
    # four cells of one dword marked by different samples: what the marks' atomic OR has to keep apart
    d = tab.reshape(-1, 4)
    assert ((d != 0).sum(1) >= 2).any()


def test_the_file_and_the_lines():
    cov = np.array([[0, 3, 0, 7], [0, 0, 0, 0], [5, 0, 0, 1]], np.uint32)
    ss = np.array([10, 11, 12, 13], np.uint32)
    assert pr.format_panel(cov, ss) == b"0\t1\t3\t11\n0\t3\t7\t13\n2\t0\t5\t10\n2\t3\t1\t13\n"
    assert pr.format_panel(cov[2:], ss, first=8) == b"8\t0\t5\t10\n8\t3\t1\t13\n"
    # sample s's lines with the first field cut off are the -C file
    assert b"".join(l.split(b"\t", 1)[1] for l in pr.format_panel(cov, ss).splitlines(True) if l.startswith(b"2\t")) == cr.format_cover(cov[2], ss)
    assert pr.sample_line(9, 20, 300, 9, 8, cov[0]) == b"panel[9]: 20 queries, 300 of 131072 cells seen, 2 genomes covered"
    assert pr.summary_line(10) == b"panel: 10 samples, 2 passes over the matrix" and pr.summary_line(8) == b"panel: 8 samples, 1 passes over the matrix"
