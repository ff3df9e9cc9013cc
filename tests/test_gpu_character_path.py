"""The build's character path and the single-query long sketches against the oracle.

At h >= 23 a sketch has more than 1,024 bins of 2^12 partitions, which the binned build does not take:
a batch goes through the atomic sketch kernel, finalize_kernel, bloom_post_kernel and the sweep instead.
Runs of long queries are refused by the same rule, so the sparse long and the dense query sketches
run one query at a time."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

K, H = 21, 23


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


@pytest.fixture(scope="module")
def genomes():
    return [synth.genome_bases(4100 + g, 0, 3000 + 37 * g) for g in range(5)]


@pytest.fixture(scope="module")
def queries(genomes):
    def around(seed, total, inserts):
        """`total` bases of filler with the genomes `inserts` spliced in, so that the query scores against them"""
        parts, left = [], total - sum(len(genomes[g]) for g in inserts)
        piece = left // (len(inserts) + 1)
        for i, g in enumerate(inserts):
            parts += [synth.genome_bases(seed + i, 0, piece), genomes[g]]
        parts.append(synth.genome_bases(seed + len(inserts), 0, total - sum(len(p) for p in parts)))
        return b"".join(parts)
    read = genomes[2][1000:1800]                       # 800 bases: the short sketch
    sparse = around(4200, 300_000, [1, 4])             # > 2^18 k-mers, < 2^h / 4: the sparse long path, single
    dense = around(4300, 2_200_000, [0, 3])            # >= 2^h / 4 k-mers: the dense path, single
    assert (1 << 18) < len(sparse) - K < (1 << H) // 4 <= len(dense) - K
    return [read, sparse, dense]


@pytest.mark.parametrize("fp_bits,b", [(8, 32), (16, 33)])
def test_character_path_build_and_single_long_queries(hip, genomes, queries, fp_bits, b):
    """Five genomes in two calls (three, then two: the second batch starts at column 3, which is no
    multiple of four, and neither batch is one of four genomes), then a read, a sparse long and a
    dense query."""
    from oracle import oracle as orc
    o = orc.OracleMiekki(K, H, fp_bits, b, 5)
    o.insert_sequences(genomes)
    ix = hip.Miekki(K, H, fp_bits, b, 5)
    try:
        ix.insert_sequences(genomes[:3])
        assert ix.index_size == 3
        ix.insert_sequences(genomes[3:])
        assert ix.index_size == 5
        np.testing.assert_array_equal(ix.sketch_size, o.sketch_size)
        np.testing.assert_array_equal(ix.genome_size, o.genome_size)
        raw = bytearray(b"".join(ix.serialize())); want = bytearray(o.serialize().tobytes())
        raw[32] = want[32] = 0
        assert bytes(raw) == bytes(want)
        del raw, want
        np.testing.assert_array_equal(ix.query_sequences(queries), o.query_sequences(queries))
    finally:
        ix.close()
