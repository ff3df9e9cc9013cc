"""`miekki -J <levels> -H <taxonomy> -O <order>`: the nested families of the indexed genomes as a taxonomy for -T and the order
for -K that makes its nodes runs of ids.  The yardsticks: the oracle's rows through tests/families_ref.py for the labels,
tests/hierarchy_ref.py for the files' bytes and the stdout line."""
import numpy as np
import pytest

import families_ref as fr
import hierarchy_ref as hr
import test_gpu_hierarchy as th
from cli_util import cli, line_of, records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the 603-genome collection of two-byte fingerprints as files and a list, its five levels, the oracle's labels"""
    n = th.Nested(16)
    d = tmp_path_factory.mktemp("hierarchy")
    for g, s in enumerate(n.c.seqs):
        (d / ("g%d.fa" % g)).write_bytes(b">g%d\n%s\n" % (g, s))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(n.G)))
    K, H, fp_bits, B, T = n.c.par
    base = ["-k", str(K), "-h", str(H), "-f", str(fp_bits - 5), "-b", str(B), "-s", str(T), "-t", "1"]
    cli(["-l", "genomes.lst", "-d", "idx.gz", "-o", "o.txt", *base], d)
    return n, d


def test_taxonomy_and_order_close_the_loop(work):
    n, d = work
    J = hr.levels_argument(n.levels)
    assert n.levels[0] == (10, 0.5 * n.c.THRESHOLD)                                      # level 0 is -F's level
    order, nodes = hr.layout(n.want)
    plain = cli(["-i", "idx.gz", "-F", "fam0.txt", "-o", "o0.txt", "-t", "1"], d).stdout
    so = cli(["-i", "idx.gz", "-J", J, "-H", "tax.txt", "-O", "order.txt", "-F", "fam.txt", "-o", "o1.txt", "-t", "1"], d).stdout
    assert (d / "fam.txt").read_bytes() == (d / "fam0.txt").read_bytes() == fr.format_labels(n.want[0])
    assert line_of(so, b"families:") == line_of(plain, b"families:") == [fr.summary_line(n.want[0])]
    assert (d / "order.txt").read_bytes() == hr.order_bytes(order)
    assert (d / "tax.txt").read_bytes() == hr.taxonomy_bytes(nodes)
    assert line_of(so, b"hierarchy:") == [hr.summary_line(n.want, nodes)]
    assert order != list(range(n.G))                                                     # (the order changes)
    # the reads: 1 kb of species A's strains and of an unrelated genome, kept when the ORACLE lists what the check needs --
    # strains of A only, more than one of them; the unrelated genome alone
    lists = lambda s: set(np.nonzero(n.a.lists(10, 0.5 * n.c.THRESHOLD, n.a.o.query_sequence(s)[0][None, :])[0])[0].tolist())
    a_set = set(n.c.species_a)
    a_reads = [r for r in (n.c.seqs[g][o:o + 1000] for g in n.c.species_a for o in (100, 900, 1700)) if len(lists(r)) > 1 and lists(r) <= a_set]
    lone = next(g for g in range(200, 260) if n.want[0][g] == g and (n.want[0] == g).sum() == 1)
    l_reads = [r for r in (n.c.seqs[lone][o:o + 1000] for o in (0, 500, 1000)) if lists(r) == {lone}]
    assert len(a_reads) >= 2 and l_reads
    (d / "reads.fa").write_bytes(records(a_reads + l_reads))
    place = {j: p for p, j in enumerate(order)}
    a_places = sorted(place[g] for g in a_set)
    a_node = [name for first, last, name, _ in nodes if name[0] == "L" and list(range(first, last + 1)) == a_places]
    assert len(a_node) == 1                                                              # species A is a node of its own
    cli(["-i", "idx.gz", "-K", "order.txt", "-d", "grouped.gz", "-o", "o2.txt", "-t", "1"], d)
    cli(["-i", "grouped.gz", "-a", "reads.fa", "-T", "tax.txt", "-y", "report.txt", "-o", "o3.txt", "-t", "1"], d)
    report = [l.split(b"\t") for l in (d / "report.txt").read_bytes().split(b"\n") if l]
    by_name = {l[8]: l for l in report}
    a_line = by_name[a_node[0].encode()]
    assert (int(a_line[2]), int(a_line[3])) == (a_places[0], a_places[-1]) and int(a_line[4]) == len(a_reads)
    leaf = by_name[b"g%d" % lone]
    assert int(leaf[2]) == int(leaf[3]) == place[lone] and int(leaf[5]) == len(l_reads)
    # on the grouped index every family of every level is a run already: the identity order
    so2 = cli(["-i", "grouped.gz", "-J", J, "-H", "tax2.txt", "-O", "order2.txt", "-o", "o4.txt", "-t", "1"], d).stdout
    assert (d / "order2.txt").read_bytes() == hr.order_bytes(range(n.G))
    moved = n.want[:, order]
    again = np.stack([[int(np.nonzero(row == l)[0][0]) for l in row] for row in moved])   # labels as the smallest NEW id
    assert (d / "tax2.txt").read_bytes() == hr.taxonomy_bytes(hr.layout(again)[1])
    assert line_of(so2, b"hierarchy:") == [hr.summary_line(again, hr.layout(again)[1])]


def test_the_flags_are_refused_before_a_device_is_touched(tmp_path):
    r = cli(["-l", "genomes.lst", "-J", "10,5", "-H", "t.txt", "-O", "o.txt"], tmp_path, ok=False)
    assert r.returncode == 1 and r.stdout.startswith(b"-J: level 1") and b"Using " not in r.stdout
    r = cli(["-l", "genomes.lst", "-J", "10", "-H", "t.txt"], tmp_path, ok=False)
    assert r.returncode == 1 and b"needs -O" in r.stdout
    r = cli(["-l", "genomes.lst", "-J", "10", "-H", "t.txt", "-O", "o.txt"], tmp_path, devices="0,0", ok=False)
    assert r.returncode == 1 and b"several GPUs" in r.stdout
    assert not any((tmp_path / f).exists() for f in ("out.txt", "t.txt", "o.txt"))
