"""What joining two indexes means (mk_index_extend, `miekki -M`): the index of ONE build of the first index's genomes
followed by the second's.  The reference's own member for it is unfinished (Miekki::merge_indexes, Miekki.cpp:901-910), so
the definition is the build itself, and this file checks on the CPU that tests/extend_ref.py: joined_stream -- numpy surgery
on the two parts' streams -- gives exactly the oracle's joint build.  Two facts carry it: a genome's column and sizes depend
on its own sequence only (Miekki.cpp:277-314), and a Bloom cell keeps the byte of its first writer in genome order
(Miekki.cpp:121-131), while a k-mer that finds an empty cell among its five always writes it."""
import numpy as np
import pytest

import extend_ref
import synth

K, H, B, THR = 21, 9, 32, 10
SHAPES = {8: (120, (1, 17, 60, 119)), 16: (60, (9, 31))}


def build(fp_bits, seqs):
    from oracle import oracle as orc
    o = orc.OracleMiekki(K, H, fp_bits, B, THR)
    o.insert_sequences(seqs)
    s = o.serialize()
    s[32] = 0
    return s


@pytest.mark.parametrize("fp_bits", sorted(SHAPES))
def test_joined_stream_is_the_joint_build(fp_bits):
    G, cuts = SHAPES[fp_bits]
    seqs = [synth.genome_bases(930_000 + 11 * G + g, 0, 2000 + 3 * (g % 37)) for g in range(G)]
    for g in range(3, G, 4):                                         # every fourth shares its first half with the one before it
        seqs[g] = seqs[g - 1][:1000] + seqs[g][1000:]
    whole = build(fp_bits, seqs)
    for c in cuts:
        a, b = build(fp_bits, seqs[:c]), build(fp_bits, seqs[c:])
        bla, blb = extend_ref.parts(a)[3], extend_ref.parts(b)[3]
        # cells both parts wrote with different bytes: a fold in the wrong direction cannot pass
        assert int(np.count_nonzero((bla != 0) & (blb != 0) & (bla != blb))) > 0, c
        got = extend_ref.joined_stream(a, b)
        assert len(got) == len(whole), c
        assert np.array_equal(got, whole), (c, int(np.flatnonzero(got != whole)[0]))
        wrong = extend_ref.joined_stream(b, a)                       # (the other order is another index)
        assert not np.array_equal(extend_ref.parts(wrong)[3], extend_ref.parts(whole)[3]), c
        del a, b, got, wrong
