"""The yardstick of the representatives tests (tests/test_representatives*.py, tests/test_gpu_representatives.py,
tests/test_gpu_cli_representatives.py): a plain Python greedy over families_ref.Answer.lists(...) -- the oracle's rows and
families_ref.passes.  Nothing here touches the code under test."""
import numpy as np

import families_ref as fr


def links(lists):
    """linked[i, j]: i != j and one of the two lists the other (lists is square: query i is genome i)"""
    lists = np.asarray(lists, bool)
    assert lists.shape[0] == lists.shape[1]
    return (lists | lists.T) & ~np.eye(len(lists), dtype=bool)


def greedy(linked):
    """rep[i] = i when no representative r < i is linked with i, else the smallest such representative"""
    n = len(linked)
    rep = np.arange(n, dtype=np.uint32)
    reps = []
    for i in range(n):
        for r in reps:                                   # ascending
            if linked[i, r]:
                rep[i] = r
                break
        else:
            reps.append(i)
    return rep


def representatives(answer, min_score=10, min_intersection=None, lo=0, hi=None):
    """the model over genomes [lo, hi) of an Answer, as local ids"""
    mi = 0.5 * answer.threshold if min_intersection is None else min_intersection
    hi = len(answer.seqs) if hi is None else hi
    return greedy(links(answer.lists(min_score, mi)[lo:hi, lo:hi]))


def check_consequences(rep, linked):
    """what the definition implies, asserted on its own"""
    rep = np.asarray(rep, np.int64)
    n = len(rep)
    assert (rep <= np.arange(n)).all()
    assert (rep[rep] == rep).all()
    reps = np.nonzero(rep == np.arange(n))[0]
    assert not linked[np.ix_(reps, reps)].any()                          # no two representatives are linked
    members = np.nonzero(rep != np.arange(n))[0]
    assert linked[members, rep[members]].all()                           # every member is linked with its representative
    for i in members:                                                    # ... and with no smaller representative
        assert not linked[i, reps[reps < rep[i]]].any()


def format_representatives(rep):
    """the bytes of `miekki -R`: the representatives, ascending"""
    return b"".join(b"%d\n" % j for j, r in enumerate(rep) if int(r) == j)


def summary_line(rep):
    sizes = np.bincount(np.asarray(rep, np.int64))
    sizes = sizes[sizes > 0]
    return b"representatives: %d of %d, largest cluster %d" % (len(sizes), len(rep), sizes.max() if len(sizes) else 0)
