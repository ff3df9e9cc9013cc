"""The clade tally's definition on the oracle alone (tests/clade_ref.py): what the map layouts of the GPU tests were cut for
holds on tests/tally_ref.Sample as it is, and the identities the header states hold on the reference's own numbers.  No GPU,
nothing of the code under test."""
import numpy as np
import pytest

import clade_ref as cr
import tally_ref as tr

THRESHOLDS = [(10, 10.0), (10, 60.0), (10, 100.0)]


@pytest.fixture(scope="module")
def sample():
    s = tr.Sample()
    return s, {(ms, mi): cr.per_query(s.o, s.rows, ms, mi) for ms, mi in THRESHOLDS}


def test_layouts_are_what_the_walks_need():
    lay = cr.layouts()
    assert set(lay) == {"single", "one", "fine", "coarse", "masked"}
    for name, clade in lay.items():
        assert len(clade) == 1101
        have = [c for c in clade if c is not None]
        assert have == sorted(have), name                                   # the one restriction
    fine = lay["fine"]
    for cut in (4, 8, 256, 512, 1000):                                      # lane boundaries of either walk, both step boundaries
        assert fine[cut - 1] != fine[cut]
    assert fine[0] != fine[1] and fine[4] != fine[5] and fine[256] != fine[257] and fine[512] != fine[513]   # cuts inside a lane
    coarse = lay["coarse"]
    assert coarse[100] == coarse[1049] == 1                                 # one clade over whole steps of both walks
    masked = lay["masked"]
    assert masked[1024] is None and masked[4] is None and masked[1023] is not None
    assert cr.n_clades(masked) == 2 * 13 + 1 and set(c for c in masked if c is not None) == {2 * c for c in range(14) if c % 3 != 2}
    assert cr.n_clades(lay["single"]) == 1101 and cr.n_clades(lay["one"]) == 1 and cr.n_clades([None] * 5) == 0


def test_preconditions_on_the_oracle_alone(sample):
    """The planted species {3, 64, 1023, 1024, 1100} and {63, 65, 519, 1044} make the layouts bite as they are: no cut had to
    be moved."""
    s, lists = sample
    lay = cr.layouts()
    fine, masked, coarse, single = lay["fine"], lay["masked"], lay["coarse"], lay["single"]
    two_of_one = two_clades = other_best = newly_unique = 0
    for (ms, mi), per in lists.items():
        for listed in per:
            cl = [fine[h[0]] for h in listed]
            two_of_one += len(cl) > len(set(cl))
            two_clades += len(set(cl)) > 1
            mine = cr.restricted(listed, masked)
            other_best += bool(mine) and cr.best_of(mine)[0] != cr.best_of(listed)[0]
            newly_unique += len({coarse[h[0]] for h in listed}) == 1 and len({single[h[0]] for h in listed}) > 1
    assert two_of_one and two_clades and other_best and newly_unique, (two_of_one, two_clades, other_best, newly_unique)
    # a list that spans more than one step of either walk inside ONE clade of `coarse`: the carry is exercised
    assert any(sum(coarse[h[0]] == 1 for h in listed) > 512 for listed in lists[10, 10.0])


@pytest.mark.parametrize("ms,mi", THRESHOLDS)
def test_identities_on_the_references_own_numbers(sample, ms, mi):
    s, lists = sample
    per = lists[ms, mi]
    G = s.c.G
    plain = tr.tally(s.o, s.rows, ms, mi)
    np.testing.assert_array_equal(cr.plain_tally(per, G), plain)            # (the lists are the tally tests' lists)
    lay = cr.layouts(G)
    single = cr.clade_tally(per, lay["single"])
    np.testing.assert_array_equal(single[:, :4], plain)
    np.testing.assert_array_equal(single[:, 4], plain[:, 0])                # hits = listed
    one = cr.clade_tally(per, lay["one"])
    assigned = sum(1 for listed in per if listed)
    assert one.shape == (1, 5) and one[0, 0] == one[0, 1] == one[0, 2] == assigned and one[0, 4] == plain[:, 0].sum()
    for name in ("fine", "coarse"):
        t = cr.clade_tally(per, lay[name])
        assert t[:, 2].sum() == plain[:, 2].sum() and t[:, 4].sum() == plain[:, 0].sum()
        assert (t[:, 1] <= t[:, 0]).all() and (t[:, 2] <= t[:, 0]).all() and (t[:, 0] <= t[:, 4]).all()
        for c in range(len(t)):                                             # hits per clade = the members' listed
            members = [g for g in range(G) if lay[name][g] == c]
            assert t[c, 4] == plain[members, 0].sum()
    masked = cr.clade_tally(per, lay["masked"])
    assert masked.shape == (27, 5) and not masked[1::2].any() and not masked[4::6].any()
    assert masked[:, 2].sum() <= plain[:, 2].sum() and masked[:, 4].sum() < plain[:, 0].sum()


def test_files_and_lines():
    lay = cr.layouts()
    text, renumbered = cr.clade_file(lay["masked"])
    assert text.startswith(b"0\n\n1\n2\n3\n\n5\n6\n7\n\n") and text.endswith(b"\n1100\n") and b"\n1024\n" not in text
    assert cr.n_clades(renumbered) == 10 and renumbered[1024] is None and renumbered[1023] == renumbered[1025]
    ids = [int(x) for x in text.split()]
    assert ids == sorted(set(ids)) and len(ids) == sum(c is not None for c in renumbered)
    t = np.array([[3, 1, 2, 40, 5], [0, 0, 0, 0, 0], [1, 1, 1, 12, 1]], np.uint64)
    assert cr.format_clade_profile(t, [0, 0, None, 1, 2, 2]) == b"0\t0\t2\t2\t1\t3\t40\t5\n2\t4\t2\t1\t1\t1\t12\t1\n"
    assert cr.summary_line(t, 9) == b"clades: 9 queries, 3 assigned, 2 listing one clade only, 2 clades listed"
