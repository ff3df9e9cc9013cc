"""`miekki -a <reads> -T <taxonomy> -U <file>`: the distinct covered cells per node of the taxonomy over query_file's
super-batches.  The yardstick is tests/taxon_cover_ref.py over the oracle's gated sketches and stored columns: the file's bytes
and the stdout line are what it formats to."""
import pytest

import cover_ref as cr
import lca_ref as lr
import synth
import taxon_cover_ref as tcr
from cli_util import cli, line_of, records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the grouped collection as a dumped index, its reads as records, the `deep` taxonomy's file and the yardstick's counts"""
    s = lr.Grouped()
    d = tmp_path_factory.mktemp("taxon_cover")
    for g, seq in enumerate(s.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.G)))
    k, h, fp_bits, b, threshold = s.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    (d / "once.fa").write_bytes(records(s.reads))
    (d / "short_mates.fa").write_bytes(records([r[:k - 1] for r in s.reads]))      # mates without a k-mer: a pair is its read alone
    nodes = lr.taxonomies(s.G)["deep"]
    tree, names = lr.Tree(nodes, s.G), lr.names_of(nodes)
    (d / "deep.txt").write_bytes(lr.taxonomy_file(nodes, names))
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    seen = cr.seen(s.o, s.reads)
    nc = tcr.node_cover(s.o, seen, cr.stored(s.o), nodes)
    return s, d, tree, names, nc, int(seen.sum())


def test_file_and_summary(work):
    s, d, tree, names, nc, cells = work
    k, h, fp_bits = s.par[:3]
    r = cli(["-i", "full.gz", "-a", "once.fa", "-T", "deep.txt", "-U", "U.txt", "-o", "o.txt", "-t", "1"], d)
    want = tcr.format_taxon_cover(nc, tree, names)
    assert want.count(b"\n") > 5
    assert (d / "U.txt").read_bytes() == want
    assert line_of(r.stdout, b"taxon cover: ") == [tcr.summary_line(len(s.reads), cells, h, fp_bits, nc)]
    assert (d / "o.txt").read_bytes() == b""


def test_beside_the_other_profiles(work):
    """-U beside -C -y -P: their files and lines are byte for byte those of a run without -U, and -U's are its own run's"""
    s, d, tree, names, nc, cells = work
    others = ["-C", "C.txt", "-T", "deep.txt", "-y", "y.txt", "-P", "P.txt"]
    alone = cli(["-i", "full.gz", "-a", "once.fa", *others, "-o", "o.txt", "-t", "1"], d)
    kept = {f: (d / f).read_bytes() for f in ("C.txt", "y.txt", "P.txt")}
    assert all(kept.values())
    for f in kept:
        (d / f).unlink()
    both = cli(["-i", "full.gz", "-a", "once.fa", *others, "-U", "U_both.txt", "-o", "o.txt", "-t", "1"], d)
    for f, text in kept.items():
        assert (d / f).read_bytes() == text, f
    for head in (b"profile: ", b"lca: ", b"cover: "):
        assert line_of(both.stdout, head) == line_of(alone.stdout, head) and len(line_of(alone.stdout, head)) == 1
    assert line_of(alone.stdout, b"taxon cover: ") == []
    assert (d / "U_both.txt").read_bytes() == tcr.format_taxon_cover(nc, tree, names)
    assert line_of(both.stdout, b"taxon cover: ") == [tcr.summary_line(len(s.reads), cells, s.par[1], s.par[2], nc)]


def test_pairs_whose_mates_hold_no_kmer(work):
    """-2 with mates shorter than k: every pair is its read alone, the file is the plain run's"""
    s, d, tree, names, nc, cells = work
    r = cli(["-i", "full.gz", "-a", "once.fa", "-2", "short_mates.fa", "-T", "deep.txt", "-U", "U_pairs.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "U_pairs.txt").read_bytes() == tcr.format_taxon_cover(nc, tree, names)
    assert line_of(r.stdout, b"taxon cover: ") == [tcr.summary_line(len(s.reads), cells, s.par[1], s.par[2], nc)]


def test_an_id_beyond_the_index(work):
    s, d, _, _, _, _ = work
    (d / "beyond.txt").write_bytes(b"0 %d all\n0 1\n" % s.G)
    r = cli(["-i", "full.gz", "-a", "once.fa", "-T", "beyond.txt", "-U", "beyond_U.txt", "-o", "o_b.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-T: line 1 of beyond.txt: genome id %d is beyond the index's %d genomes" % (s.G, s.G) in r.stdout
    assert not (d / "beyond_U.txt").exists() and b"taxon cover: " not in r.stdout
