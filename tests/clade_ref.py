"""The yardstick of the clade tally tests (tests/test_clade_definition.py, tests/test_gpu_clade_tally.py,
tests/test_gpu_cli_clades.py): per query the oracle's own filter_results over its score row -- the full list with its
intersections -- restricted to the genomes that have a clade, best' = the maximum of (intersection, id) over that restricted
list, summed per clade in Python integers.  Nothing here touches the code under test."""
import numpy as np

COLUMNS = ("listed", "unique", "best", "best_matches", "hits")
NO_CLADE = 0xffffffff
FINE = (0, 1, 4, 5, 8, 100, 255, 256, 257, 511, 512, 513, 1000, 1050, 1101)
COARSE = (0, 100, 1050, 1101)


def from_cuts(cuts):
    """clade i = the genomes [cuts[i], cuts[i + 1])"""
    clade = []
    for i in range(len(cuts) - 1):
        clade += [i] * (cuts[i + 1] - cuts[i])
    return clade


def layouts(G=1101):
    """name -> a clade number or None (left out) per genome.  The walk steps 256 genomes at 4 per lane on scores and 512 at 8
    per lane on partial counts: `fine` cuts at lane boundaries, inside lanes and at both kernels' step boundaries; a clade
    of `coarse` spans several whole steps (the carry); `masked` is `fine` with every third clade and genome 1024 left out and
    the numbers doubled (left-out genomes, gaps in the numbering)."""
    assert G == FINE[-1] == COARSE[-1]
    fine = from_cuts(FINE)
    masked = [None if c % 3 == 2 or g == 1024 else 2 * c for g, c in enumerate(fine)]
    return {"single": list(range(G)), "one": [0] * G, "fine": fine, "coarse": from_cuts(COARSE), "masked": masked}


def n_clades(clade):
    return 1 + max((c for c in clade if c is not None), default=-1)


def as_u32(clade):
    return np.array([NO_CLADE if c is None else c for c in clade], np.uint32)


def per_query(o, rows, ms, mi):
    """[[(id, matches, intersection) of every genome the query lists, ascending id]] from the oracle's filter_results alone;
    asserted once, on the oracle alone: the maximum of (intersection, id) over the full list is filter_results(row, 1, ...)"""
    out = []
    for row in rows:
        full = sorted((h[0], h[1], h[3]) for h in o.filter_results(row, o.index_size, ms, mi))
        one = o.filter_results(row, 1, ms, mi)
        assert len(one) == min(1, len(full))
        if full:
            assert best_of(full)[:2] == (one[0][0], one[0][1])
        out.append(full)
    return out


def best_of(listed):
    """the largest intersection, among equals the largest id"""
    return max(listed, key=lambda h: (h[2], h[0]))


def restricted(listed, clade):
    return [h for h in listed if clade[h[0]] is not None]


def clade_tally(lists, clade):
    """uint64 [n_clades, 5]: listed, unique, best, best_matches, hits per clade over the queries whose lists (per_query) are
    `lists`, in Python integers"""
    t = [[0] * 5 for _ in range(n_clades(clade))]
    for listed in lists:
        mine = restricted(listed, clade)
        if not mine:
            continue
        seen = {clade[h[0]] for h in mine}
        for c in seen:
            t[c][0] += 1
        if len(seen) == 1:
            t[next(iter(seen))][1] += 1
        b = best_of(mine)
        t[clade[b[0]]][2] += 1
        t[clade[b[0]]][3] += b[1]
        for h in mine:
            t[clade[h[0]]][4] += 1
    return np.array(t, np.uint64).reshape(len(t), 5)


def plain_tally(lists, G):
    """the plain tally (tests/tally_ref.py's columns) from the same lists: uint64 [G, 4]"""
    t = np.zeros((G, 4), np.uint64)
    for listed in lists:
        for h in listed:
            t[h[0], 0] += 1
        if len(listed) == 1:
            t[listed[0][0], 1] += 1
        if listed:
            b = best_of(listed)
            t[b[0], 2] += 1
            t[b[0], 3] += b[1]
    return t


def clade_file(clade):
    """(the bytes of a -L file, the map it stands for): -F's layout -- ids one per line, a blank line between clades -- for the
    genomes that have a clade; the file's clade numbers are its blocks' indices, so the map is `clade` renumbered from 0
    without gaps"""
    blocks, renumbered, last = [], [], None
    for g, c in enumerate(clade):
        if c is None:
            renumbered.append(None)
            continue
        if last is None or c != last:
            blocks.append([])
            last = c
        blocks[-1].append(g)
        renumbered.append(len(blocks) - 1)
    return b"\n".join(b"".join(b"%d\n" % g for g in blk) for blk in blocks), renumbered


def format_clade_profile(t, clade):
    """the bytes of `miekki -p`: a line per clade somebody lists, ascending: clade, first id, members, best, unique, listed,
    best_matches, hits"""
    first, members = {}, {}
    for g, c in enumerate(clade):
        if c is not None:
            first.setdefault(c, g)
            members[c] = members.get(c, 0) + 1
    return b"".join(b"%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (c, first[c], members[c], int(r[2]), int(r[1]), int(r[0]), int(r[3]), int(r[4]))
                    for c, r in enumerate(t) if int(r[0]))


def summary_line(t, n_queries):
    t = np.asarray(t)
    return b"clades: %d queries, %d assigned, %d listing one clade only, %d clades listed" % (
        n_queries, int(t[:, 2].sum()), int(t[:, 1].sum()), int((t[:, 0] > 0).sum()))
