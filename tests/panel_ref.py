"""The yardstick of the panel tests (tests/test_gpu_panel.py, tests/test_gpu_cli_panel.py, tests/test_panel_definition.py): the
expected table -- bit s of byte (p << fp_bits) + v set iff sample s's cover has seen(p, v) -- and the per-slot counts, both built
on tests/cover_ref.py and so on the oracle's gated sketches and stored columns; the bytes of `miekki -S ... -c` and its stdout
lines.  Nothing here touches the code under test."""
import numpy as np

import cover_ref as cr

SLOTS = 8


def deal(s):
    """a tr.Sample's queries dealt into eight samples of unlike sizes: one empty, one of a single read, one of whole genomes
    and genomes in a row (dense queries at -h 9); the others runs of reads, two of which overlap"""
    r, g = s.reads, s.c.seqs
    dense = [g[7] + g[8], g[3] * 2, g[64]]
    assert all(len(x) > s.c.K + 4096 for x in dense[:2])
    return [r[:200], r[200:210], [], r[210:211], r[211:400], dense, r[400:], r[150:260]]


def seen_per_sample(o, samples):
    """[bool [P, 2^fp_bits]] per sample: cr.seen of its queries"""
    return [cr.seen(o, q) for q in samples]


def table(seens):
    """uint8 [P * 2^fp_bits]: sum_s seen_s << s, for at most eight samples"""
    assert 0 < len(seens) <= SLOTS
    t = np.zeros(seens[0].shape, np.uint8)
    for s, seen in enumerate(seens):
        t |= seen.astype(np.uint8) << np.uint8(s)
    return t.reshape(-1)


def plane(tab, slot, P, fp_bits):
    """bool [P, 2^fp_bits]: slot `slot` of a table"""
    return ((np.asarray(tab, np.uint8) >> np.uint8(slot)) & 1).astype(bool).reshape(P, 1 << fp_bits)


def covered(o, seens, fps=None):
    """uint32 [n, G]: cr.covered per sample"""
    fps = cr.stored(o) if fps is None else fps
    return np.stack([cr.covered(o, seen, fps) for seen in seens]) if seens else np.zeros((0, o.index_size), np.uint32)


def cells(seens):
    return np.array([int(seen.sum()) for seen in seens], np.uint64)


def count_table(o, tab, n_slots, fps=None):
    """(covered uint32 [n_slots, G], cells uint64 [n_slots]) of any table of bytes"""
    P, bits = o.P, o.number_bit_minimizer
    seens = [plane(tab, s, P, bits) for s in range(n_slots)]
    return covered(o, seens, fps), cells(seens)


def format_panel(cov, sketch_size, first=0):
    """the bytes of `miekki -S ... -c`: a line per (sample, genome) with covered > 0, samples ascending, ids ascending within a
    sample: sample, id, covered, sketch_size"""
    return b"".join(b"%d\t" % (first + s) + line for s, row in enumerate(cov) for line in cr.format_cover(row, sketch_size).splitlines(True))


def sample_line(sample, n_queries, n_cells, h, fp_bits, cov_row):
    return b"panel[%d]: %d queries, %d of %d cells seen, %d genomes covered" % (
        sample, n_queries, int(n_cells), 1 << (h + fp_bits), int((np.asarray(cov_row) > 0).sum()))


def summary_line(n_samples):
    return b"panel: %d samples, %d passes over the matrix" % (n_samples, (n_samples + SLOTS - 1) // SLOTS)
