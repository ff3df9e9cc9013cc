"""The query-block scan's PAIR WORDS (scan_kernel.hpp: pair_word): block_list_kernel writes a pair as the word that
scan_block_kernel consumes -- at one-byte fingerprints `fingerprint << 24 | byte offset of the slot's counters in LDS`, at
two bytes `slot << 16 | fingerprint` -- and the kernel takes the broadcast fingerprint and the counters' address out of it
with one instruction each.  What can go wrong is a field that leaks into the other (a slot offset that reaches the
fingerprint's byte, a fingerprint bit that moves the address), an address that is right for some slots only (the lane's
offset is OR-ed into the slot's), and -- should the slots' counters ever be spread over the LDS banks by the slot number --
packets whose slots agree or differ mod 4.

The helpers, the knobs and the three paths (the block kernel against the oracle, against the query groups' kernel and
against the one-query-per-wave kernel) are test_gpu_scan_block_lanes.py's.
"""
import pytest

import synth
from test_gpu_scan_block_lanes import build, check, queries_of
from test_gpu_scan_block_lanes import range_table_path, small_blocks  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LDS_BYTES = 160 << 10          # a CU's LDS, all of which a default block's counters fill
SLOT_PITCH = 128               # bytes from a slot's counters to the next slot's: the 128-byte sub-tile
BLOCK_Q = LDS_BYTES // SLOT_PITCH


@pytest.mark.parametrize("fpb", [8, 16])
def test_copies_at_slot_distances_1_4_8(monkeypatch, small_blocks, fpb):
    """Blocks of 24.  Three queries per block are present four times, at slots s, s + 1, s + 4 and s + 8 (s = 0, 2, 11);
    two more twice, at distance 4 (slots 5, 9: they agree mod 4) and at distance 1 (13, 14: they differ).  Identical queries
    want the same partitions: those of the fourfold ones have a packet of three pairs and one of one pair, those of the
    twofold ones packets of two, and the slots inside a packet both agree and differ mod 4.  54 queries are two blocks and
    a short one; the second block repeats the pattern with other sequences.  Every copy's hits are the original's, and
    the oracle's (check)."""
    G, L, qlen = 40, 40_000, 700
    ix, ref = build(21, 12, fpb, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, 54, qlen)
        same = []
        for b in (0, 24):
            for s, dists in ((0, (1, 4, 8)), (2, (1, 4, 8)), (11, (1, 4, 8)), (5, (4,)), (13, (1,))):
                for d in dists:
                    qs[b + s + d] = qs[b + s]
                    same.append((b + s, b + s + d))
        assert len(set(qs)) == 54 - len(same)
        exp = check(ix, ref, qs, monkeypatch, ms=10, mi=10.0)
        assert any(exp[o] for o, _ in same)
        for o, c in same:
            assert exp[c] == exp[o], (o, c)
    finally:
        ix.close()


@pytest.mark.parametrize("G", [17, 129, 144, 260])
def test_fields_of_a_pair_word_at_the_ends_of_a_full_block(monkeypatch, G):
    """No block knobs: BLOCK_Q + 5 queries of 100 bases are one full default block -- its last slot's counters end with the
    LDS, its offset is the largest a pair word ever holds -- and a block of five.  The queries at slot 0 and at the last
    slot of each residue mod 4 (BLOCK_Q - 1 ... BLOCK_Q - 4) are one sequence cut from the last genome: five pairs per
    partition, i.e. a packet of three and one of two whose slots differ mod 4, at both ends of the offset's range; slot 1
    and slot 0 of the second block are cut from genome 0.  With 17, 129 and 144 genomes those packets meet lanes that have
    no genomes (one live lane and a byte, a sub-tile of one byte, a sub-tile of one lane); the 260 random genomes' rows hold
    every byte value beside the bytes that match, so that every fingerprint difference -- 0x00, 0x01, 0x7f, 0x80, 0xff
    among them -- is compared next to a counter that must not move."""
    L, qlen = 6000, 100
    ix, ref = build(21, 12, 8, [synth.genome_bases(g, 0, L) for g in range(G)])
    try:
        qs = queries_of(G, L, BLOCK_Q + 5, qlen)
        last = synth.genome_bases(G - 1, 1234, qlen)
        ends = [0] + [BLOCK_Q - 1 - i for i in range(4)]
        for q in ends:
            qs[q] = last
        first = synth.genome_bases(0, 2345, qlen)
        for q in (1, BLOCK_Q):
            qs[q] = first
        exp = check(ix, ref, qs, monkeypatch)
        for q in ends:
            assert exp[q] and exp[q][0][0] == G - 1 and exp[q] == exp[0], q
        for q in (1, BLOCK_Q):
            assert exp[q] and exp[q][0][0] == 0 and exp[q] == exp[1], q
    finally:
        ix.close()
