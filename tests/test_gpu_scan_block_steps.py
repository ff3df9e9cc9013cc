"""The query-block scan (scan_block_kernel) at the edges of its STEPS.  A (block, range) list is padded with zero packets
to whole steps of 512 packets -- 128 lane groups x 4 packets -- and the kernel's loop knows neither a ragged last step nor
dead lanes: a lane whose bytes begin at or past the last genome is given live bytes to load, and adds into counter cells
that are never stored.  The cases are the lists at which that can go wrong: no packet, one, one short of a step, a step,
one more, two steps exactly, a few three-pair packets past a step (a window lays its one-pair packets first, so the padding
then directly follows three-pair packets), a list that ends one packet short of a step beside a list that begins with a
three-pair packet (a padded list must not reach into its neighbour), and lists of two steps against collections whose
last lanes are dead.

-k 21 -h 12 under MIEKKI_SLAB_MIB=1 is four ranges of 1,024 partitions, each one window of block_list_kernel; blocks are 24
queries.  Every case first computes, from the oracle's gated partitions (scan_limits.gated_partitions), the packet count of
every (block, range) before padding -- the sum over the range's partitions of ceil(pairs / 3) -- and asserts that the
intended counts occur; then test_gpu_scan_block_lanes.py's check compares the block kernel with the oracle and with both
other kernels.  c copies of a steered query (scan_limits.steered) with n partitions in a range are n x ceil(c / 3) packets
there, whatever the other ranges get."""
import functools

import numpy as np
import pytest

import scan_limits as sl
import synth
from test_gpu_scan_block_lanes import build, check, queries_of, range_table_path, small_blocks  # noqa: F401  (fixtures)
from test_gpu_scan_block_lanes import orc

pytestmark = pytest.mark.gpu

K, H, S, B, STEP = 21, 12, 4, 24, 512


@functools.lru_cache(maxsize=None)
def steered(fpb, r, want, seed):
    bare = orc.OracleMiekki(K, H, fpb, sl.BLOOM_LOG2, sl.THRESHOLD)
    return sl.steered(bare, S, r, want, seed)


def kmer_partitions(fpb, seq):
    """The partition of every k-mer of seq that a sketch counts (the last one is skipped), in order."""
    bare = orc.OracleMiekki(K, H, fpb, sl.BLOOM_LOG2, sl.THRESHOLD)
    return [sl.kmer_partition(bare, seq[i:i + K]) for i in range(len(seq) - K)]


def packet_lists(ref, queries):
    """[block][range] -> (packets of one pair, of two, of three) before padding, in the order a window lays them down."""
    cache, out = {}, []
    for b0 in range(0, len(queries), B):
        pairs = np.zeros(ref.P, np.int64)
        for q in queries[b0:b0 + B]:
            if q not in cache:
                cache[q] = sl.gated_partitions(ref, q) if len(q) > K else np.zeros(0, np.int64)
            pairs[cache[q]] += 1                                     # (a query's partitions are distinct)
        row = []
        for r in range(S):
            lo, hi = sl.range_bounds(ref.P, S, r)
            c = pairs[lo:hi]
            row.append((int((c % 3 == 1).sum()), int((c % 3 == 2).sum()), int((c // 3).sum())))
        out.append(row)
    return out


def totals(lists):
    return np.array([[sum(x) for x in row] for row in lists])


def few_over_a_step(fpb, r):
    """Three queries whose packets in range r are a step and a few, the few being the packets of three pairs: two steered
    sequences of 255 partitions in the range and a prefix of a third.  A prefix one base longer adds one k-mer, that is at
    most one partition: new to all three (one packet more), known to one of the others (none more) or to both (a three-pair
    packet more).  So (packets - 512 - three-pair packets) moves by at most one per base, starts below zero and ends above
    it: the first prefix at which it is zero with a three-pair packet is taken."""
    a, b, c = (steered(fpb, r, 255, 7000 + 10 * r + i) for i in range(3))
    lo, hi = sl.range_bounds(1 << H, S, r)
    in_r = lambda seq: [p for p in kmer_partitions(fpb, seq) if p is not None and lo <= p < hi]
    pa, pb, have = set(in_r(a)), set(in_r(b)), set()
    cparts = kmer_partitions(fpb, c)
    for i, p in enumerate(cparts):
        if p is not None and lo <= p < hi:
            have.add(p)
        three = len(pa & pb & have)
        if three >= 1 and len(pa | pb | have) - STEP == three:
            return a, b, c[:i + K + 1], c                            # (one more character, so that k-mer i counts)
    raise AssertionError("no prefix gives a step and its three-pair packets")


@pytest.mark.parametrize("fpb", [8, 16])
def test_steps_of_a_list(monkeypatch, small_blocks, fpb):
    """Seven blocks of 24 queries against 40 genomes, the steered sequences among them (every entry then passes the gate):
      block 0   one query of one k-mer, 23 empty ones: a list of 1 packet, lists of 0
      block 1   21 copies of 73 partitions in range 1: 7 x 73 = 511 packets, all of three pairs -- as are those of the same
                block's range 2, the NEXT list in the buffer, which so begins with a three-pair packet behind one packet of padding
      block 2   12 copies of 128 partitions in range 2: 4 x 128 = 512
      block 3   9 copies of 171 partitions in range 0: 3 x 171 = 513
      block 4   24 copies of 128 partitions in range 3: 8 x 128 = 1,024, two steps exactly
      block 5   few_over_a_step in range 1: 512 packets of one and two pairs, then a few of three
      block 6   ordinary queries, one cut from genome 0 and one from the last genome: both must come back on top."""
    G, L = 40, 6000
    s73, s128, s171, t128 = steered(fpb, 1, 73, 11), steered(fpb, 2, 128, 12), steered(fpb, 0, 171, 13), steered(fpb, 3, 128, 14)
    fa, fb, fc_prefix, fc = few_over_a_step(fpb, 1)
    genomes = [synth.genome_bases(g, 0, L) for g in range(G)]
    for at, seq in zip((3, 9, 14, 20, 25, 26, 31), (s73, s128, s171, t128, fa, fb, fc)):
        genomes[at] = seq
    at = next(i for i, p in enumerate(kmer_partitions(fpb, genomes[5][:200])) if p is not None)
    tiny = genomes[5][at:at + K + 1]                                     # one k-mer that a sketch keeps (and the character after it)
    ordinary = queries_of(G, L, B, 500)
    ordinary[4] = synth.genome_bases(0, 700, 500)
    ordinary[17] = synth.genome_bases(G - 1, 900, 500)
    qs = ([tiny] + [b""] * 23 + [s73] * 21 + [b""] * 3 + [s128] * 12 + [b""] * 12 + [s171] * 9 + [b""] * 15 + [t128] * 24
          + [fa, fb, fc_prefix] + [b""] * 21 + ordinary)
    assert len(qs) == 7 * B and max(len(q) for q in qs) - K <= S * sl.HOST_MEAN      # (the host keeps S = 4)
    ix, ref = build(K, H, fpb, genomes, bloom=sl.BLOOM_LOG2)
    try:
        lists = packet_lists(ref, qs)
        n = totals(lists)
        assert sorted(n[0]) == [0, 0, 0, 1]
        assert n[1][1] == STEP - 1 and lists[1][1][:2] == (0, 0)
        assert lists[1][2][2] >= 1 and lists[1][2][:2] == (0, 0)            # the next list: three-pair packets only
        assert n[2][2] == STEP and n[3][0] == STEP + 1 and n[4][3] == 2 * STEP
        one, two, three = lists[5][1]
        assert one + two == STEP and 1 <= three <= 24, lists[5][1]
        exp = check(ix, ref, qs, monkeypatch)
        assert exp[6 * B + 4][0][0] == 0 and exp[6 * B + 17][0][0] == G - 1
        for q, at in ((B, 3), (2 * B, 9), (3 * B, 14), (4 * B, 20)):          # a steered query finds itself
            assert exp[q][0][0] == at, q
    finally:
        ix.close()


@pytest.mark.parametrize("fpb", [8, 16])
def test_padding_next_to_data(monkeypatch, small_blocks, fpb):
    """Two consecutive lists of the packet buffer, (block 0, range 1) and (block 0, range 2), and nothing else in the block:
    21 copies of 73 partitions in range 1 are 511 packets, one short of a step, and the copies' partitions in range 2 are
    packets of three pairs only, so the list behind the one packet of padding begins with a three-pair packet.  Block 1 is
    ordinary queries; its first list follows block 0's last."""
    G, L = 24, 6000
    s73 = steered(fpb, 1, 73, 11)
    genomes = [synth.genome_bases(g, 0, L) for g in range(G)]
    genomes[7] = s73
    qs = [s73] * 21 + [b""] * 3 + queries_of(G, L, B, 500)
    ix, ref = build(K, H, fpb, genomes, bloom=sl.BLOOM_LOG2)
    try:
        lists = packet_lists(ref, qs)
        assert sum(lists[0][1]) == STEP - 1 and lists[0][1][:2] == (0, 0)
        assert lists[0][2][2] >= 1 and lists[0][2][:2] == (0, 0)
        assert all(sum(x) > 0 for x in lists[1])
        exp = check(ix, ref, qs, monkeypatch)
        assert exp[0][0][0] == 7
    finally:
        ix.close()


@pytest.mark.parametrize("fpb,G", [(fpb, G) for fpb in (8, 16) for G in (17, 129, 144, 1025)])
def test_dead_lanes_without_guards(monkeypatch, small_blocks, fpb, G):
    """Collections that end one genome into a lane's 16 bytes, into a second sub-tile and into a second tile, and 16 genomes
    into a second sub-tile: the last sub-tile's other lanes are dead, and load and add like the live ones.  Block 0 holds
    nine copies of 171 partitions in range 0 -- 513 packets and more with the ordinary queries beside them, at least two
    steps -- and a query cut from the last genome, block 1 one cut from genome 0: each must come back on top, and no query's
    hits may differ between the three kernels (check)."""
    L, qlen = 3000, 400
    s171 = steered(fpb, 0, 171, 13)
    genomes = [synth.genome_bases(g, 0, L) for g in range(G)]
    genomes[1] = s171
    qs = [s171] * 9 + queries_of(G, L, 2 * B - 9, qlen)
    qs[11] = synth.genome_bases(G - 1, 1500, qlen)
    qs[B + 2] = synth.genome_bases(0, 800, qlen)
    ix, ref = build(K, H, fpb, genomes, bloom=sl.BLOOM_LOG2)
    try:
        n = totals(packet_lists(ref, qs))
        assert n[0][0] > STEP, n
        exp = check(ix, ref, qs, monkeypatch)
        assert exp[0][0][0] == 1 and exp[11][0][0] == G - 1 and exp[B + 2][0][0] == 0
    finally:
        ix.close()
