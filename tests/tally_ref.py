"""The yardstick of the tally tests (tests/test_gpu_tally.py, tests/test_gpu_cli_tally.py): per query the oracle's own
filter_results over its score row -- with nresults = index size for the genomes the query lists, with nresults = 1 for its best
one -- summed per genome in Python integers.  Nothing here touches the code under test."""
import numpy as np

import families_ref as fr
import synth

COLUMNS = ("listed", "unique", "best", "best_matches")


def per_query(o, rows, ms, mi):
    """[(ids the query lists, (best id, its matches) or None)] from the oracle's filter_results alone"""
    out = []
    for row in rows:
        full = o.filter_results(row, o.index_size, ms, mi)
        one = o.filter_results(row, 1, ms, mi)
        assert len(one) == min(1, len(full))
        out.append((sorted(h[0] for h in full), (one[0][0], one[0][1]) if one else None))
    return out


def tally(o, rows, ms, mi):
    """uint64 [G, 4]: listed, unique, best, best_matches per genome over the queries whose score rows are `rows`"""
    t = np.zeros((o.index_size, 4), np.uint64)
    for listed, best in per_query(o, rows, ms, mi):
        for g in listed:
            t[g, 0] += 1
        if len(listed) == 1:
            t[listed[0], 1] += 1
        if best is not None:
            t[best[0], 2] += 1
            t[best[0], 3] += best[1]
    return t


def format_profile(t, id_base=0):
    """the bytes of `miekki -P`: a line per genome somebody lists, ascending id: id, best, unique, listed, best_matches"""
    return b"".join(b"%d\t%d\t%d\t%d\t%d\n" % (j + id_base, int(r[2]), int(r[1]), int(r[0]), int(r[3]))
                    for j, r in enumerate(t) if int(r[0]))


def summary_line(t, n_queries):
    t = np.asarray(t)
    return b"profile: %d queries, %d assigned, %d listing one genome only, %d genomes listed" % (
        n_queries, int(t[:, 2].sum()), int(t[:, 1].sum()), int((t[:, 0] > 0).sum()))


class Sample:
    """fr.Collection(1101, 8, 310_000) at -k 15 -h 9 and 628 queries of it: 600 reads of 300-999 bases cut from its genomes
    (every third from a planted relative), 20 unrelated reads, eight whole genomes -- short, long and whole-genome queries:
    a mixed set.  The oracle's rows of all of them, once."""

    WHOLE = (3, 64, 1023, 1024, 1100, 10, 130, 1029)

    def __init__(self, G=1101, fp_bits=8, seed=310_000, whole=WHOLE):
        self.c = c = fr.Collection(G, fp_bits, seed)
        self.a = fr.Answer(c.par, c.seqs)
        self.o = self.a.o
        rng = np.random.default_rng(5)
        planted = c.species_a + c.species_b + c.chain + c.nested
        reads = []
        for i in range(600):
            g = int(rng.integers(0, G)) if i % 3 else int(rng.choice(planted))
            L = 300 + (i * 7) % 700
            off = int(rng.integers(0, max(1, len(c.seqs[g]) - L)))
            reads.append(c.seqs[g][off:off + L])
        reads += [synth.genome_bases(4_000_000 + i, 0, 800) for i in range(20)]
        self.reads = reads                                       # the 2-line records of the command-line tests
        self.queries = reads + [c.seqs[g] for g in whole]
        self.rows = self.o.query_sequences(self.queries)
        self.read_rows = self.rows[:len(reads)]
