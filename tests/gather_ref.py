"""The yardstick of the gather tests (tests/test_gather_definition.py, tests/test_gpu_gather.py, tests/test_gpu_cli_gather.py):
the greedy set cover as a plain numpy loop on top of cover_ref's seen, stored and covered -- count what every genome still
explains, take the first maximum (np.argmax: the smallest id among equals), strike its live cells, again.  Nothing here touches
the code under test."""
import numpy as np

import cover_ref as cr

PICK = np.dtype([("genome", np.uint32), ("fresh", np.uint32), ("covered", np.uint32), ("sketch_size", np.uint32), ("depth_sum", np.uint64)])


def loop(P, G, bits, seen_table, fps, min_new=1, max_picks=0, covered=None):
    """the definition: [(genome, fresh, flat indexes (p << bits) + v of the cells struck, genomes that shared the maximum)] per
    pick.  covered(live) -> rem [G]; the default counts as cover_ref.covered does."""
    assert min_new >= 1
    empty, parts = (1 << bits) - 1, np.arange(P)
    if covered is None:
        def covered(live):
            return (live[parts[:, None], fps] & (fps != empty)).sum(0)
    live = np.array(seen_table, bool)
    out = []
    while True:
        rem = covered(live)
        g = int(np.argmax(rem))
        fresh = int(rem[g])
        if fresh < min_new or (max_picks and len(out) == max_picks):
            return out
        col = fps[:, g]
        p = np.nonzero((col != empty) & live[parts, col])[0]
        assert len(p) == fresh
        live[p, col[p]] = False
        out.append((g, fresh, (p.astype(np.int64) << bits) + col[p], int((rem == fresh).sum())))


def picks_of(rounds, rem0, sketch_size, table=None, base=0):
    """the rounds as the library reports them: PICK records; table: uint8 [P << bits] (depth_ref.table) or None"""
    out = np.zeros(len(rounds), PICK)
    for i, (g, fresh, cells, _) in enumerate(rounds):
        out[i] = (g + base, fresh, int(rem0[g]), int(sketch_size[g]), int(np.asarray(table)[cells].astype(np.int64).sum()) if table is not None else 0)
    return out


def gather(o, seen_table, fps=None, min_new=1, max_picks=0, table=None, base=0):
    """(picks, cells, explained) of a table of seen cells against the oracle's index"""
    fps = cr.stored(o) if fps is None else fps
    rounds = loop(o.P, o.index_size, o.number_bit_minimizer, seen_table, fps, min_new, max_picks,
                  covered=lambda live: cr.covered(o, live, fps))
    picks = picks_of(rounds, cr.covered(o, seen_table, fps), o.sketch_size, table, base)
    return picks, int(np.asarray(seen_table).sum()), int(picks["fresh"].sum())


class Run:
    """the uncapped run at min_new 1 of a winners_ref.Sample, made once; every other (min_new, max_picks) is a prefix of it
    (tests/test_gather_definition.py checks that against runs of their own)"""

    def __init__(self, w):
        self.w = w
        self.rounds = loop(w.P, w.G, w.bits, w.seen, w.fps, covered=lambda live: cr.covered(w.o, live, w.fps))
        self.tie_rounds = sum(1 for r in self.rounds if r[3] > 1)

    def picks(self, min_new=1, max_picks=0, table=None, base=0):
        n = sum(1 for r in self.rounds if r[1] >= min_new)              # (fresh never increases: a prefix)
        n = min(n, max_picks) if max_picks else n
        picks = picks_of(self.rounds[:n], self.w.cov, self.w.o.sketch_size, table, base)
        return picks, self.w.cells, int(picks["fresh"].sum())


def runs(samples):
    """get(bits) -> Run of samples(bits), made on demand"""
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Run(samples(bits))
        return made[bits]
    return get


def format_gather(picks, with_depth=False):
    """the bytes of `miekki -G`: a line per pick, in pick order: id, fresh, covered, sketch_size -- and depth_sum beside -D"""
    if with_depth:
        return b"".join(b"%d\t%d\t%d\t%d\t%d\n" % (int(x["genome"]), int(x["fresh"]), int(x["covered"]), int(x["sketch_size"]), int(x["depth_sum"])) for x in picks)
    return b"".join(b"%d\t%d\t%d\t%d\n" % (int(x["genome"]), int(x["fresh"]), int(x["covered"]), int(x["sketch_size"])) for x in picks)


def summary_line(n_queries, explained, cells, n_picks, min_new):
    return b"gather: %d queries, %d of %d seen cells explained by %d genomes, each at least %d new" % (
        n_queries, int(explained), int(cells), int(n_picks), int(min_new))
