"""The winner-takes-all screen on the oracle alone (tests/winners_ref.py): what the definition promises, and that the samples of
tests/test_gpu_winners.py stay what those tests need them to be -- contested cells, ties on the share, genomes that lose cells."""
import numpy as np
import pytest

import cover_ref as cr
import synth
import winners_ref as wr


@pytest.fixture(scope="module")
def samples():
    return wr.samples()


@pytest.mark.parametrize("bits", [8, 16])
def test_invariants_and_inputs(samples, bits):
    w = samples(bits)
    o, cov, won = w.o, w.cov.astype(np.int64), w.won.astype(np.int64)
    assert sorted(w.order.tolist()) == list(range(w.G))
    assert (won <= cov).all()
    assert won[w.order[0]] == cov[w.order[0]]
    assert w.claimed == won.sum() and w.claimed <= min(w.cells, int(cov.sum()))
    # claimed, said another way: the distinct live (p, v) of the matrix that are seen
    live = w.fps != cr.empty_of(o)
    held = np.zeros_like(w.seen)
    held[np.nonzero(live)[0], w.fps[live]] = True
    assert w.claimed == int((held & w.seen).sum())
    several, ties = wr.contested(o, w.seen, w.fps, cov, w.order)
    losers = int((won != cov).sum())
    print("cells", w.cells, "claimed", w.claimed, "several holders", several, "ties", ties, "won != covered", losers, "of", w.G)
    if bits == 8:
        assert several >= 10_000 and ties >= 100
    else:
        assert several >= 1_000 and losers >= 100


def test_the_order_is_the_definition(samples):
    """neighbours in the order, by the three rules in Python integers"""
    w = samples(8)
    cov, ss = w.cov, w.o.sketch_size
    for a, b in zip(w.order[:-1].tolist(), w.order[1:].tolist()):
        left, right = int(cov[a]) * max(int(ss[b]), 1), int(cov[b]) * max(int(ss[a]), 1)
        assert left > right or (left == right and (cov[a] > cov[b] or (cov[a] == cov[b] and a < b)))


@pytest.mark.parametrize("bits", [8, 16])
def test_a_genome_queried_with_itself_keeps_all_its_cells(samples, bits):
    w = samples(bits)
    o, g = w.o, 200                                                # an unrelated genome
    seen = cr.seen(o, [w.s.c.seqs[g]])
    cov = cr.covered(o, seen, w.fps)
    order = wr.order(cov, o.sketch_size)
    won, claimed = wr.won(o, seen, w.fps, order)
    assert order[0] == g and cov[g] == o.sketch_size[g] > 0
    assert won[g] == cov[g] == claimed == seen.sum()               # every cell of the query is its own, and it wins them all
    assert not won[np.arange(w.G) != g].any()


def test_of_two_identical_genomes_the_smaller_id_wins():
    from oracle import oracle as orc
    seqs = [synth.genome_bases(910_000 + g, 0, 2500) for g in range(6)]
    seqs[4] = seqs[1]
    o = orc.OracleMiekki(15, 9, 8, 32, 20)
    o.insert_sequences(seqs)
    fps = cr.stored(o)
    seen = cr.seen(o, [seqs[1][300:1800], seqs[5][:900]])
    cov = cr.covered(o, seen, fps)
    order = wr.order(cov, o.sketch_size)
    won, claimed = wr.won(o, seen, fps, order)
    assert cov[1] == cov[4] > 0 and order.tolist().index(1) + 1 == order.tolist().index(4)
    assert won[4] == 0 and won[1] > 0
    assert claimed == won.sum()
