"""`miekki -a <reads> -T <taxonomy> -V <file>`: the taxon-specific cells over query_file's super-batches.  The yardstick is
tests/markers_ref.py over the oracle's gated sketches and stored columns: the file's bytes and the stdout line are what it
formats to; beside the other sinks their files and lines are those of a run without -V."""
import pytest

import cover_ref as cr
import lca_ref as lr
import markers_ref as mr
import synth
from cli_util import cli, line_of, records

pytestmark = pytest.mark.gpu


def fastq(reads):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the grouped collection as a dumped index, its reads as records, two taxonomy files and the yardstick's counts"""
    s = lr.Grouped()
    d = tmp_path_factory.mktemp("markers")
    for g, seq in enumerate(s.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.G)))
    k, h, fp_bits, b, threshold = s.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    (d / "once.fa").write_bytes(records(s.reads))
    (d / "once.fq").write_bytes(fastq(s.reads))
    (d / "short_mates.fa").write_bytes(records([r[:k - 1] for r in s.reads]))      # mates without a k-mer: a pair is its read alone
    seen, fps = cr.seen(s.o, s.reads), cr.stored(s.o)
    made = {}
    for name in ("deep", "masked"):
        nodes = lr.taxonomies(s.G)[name]
        tree, names = lr.Tree(nodes, s.G), lr.names_of(nodes)
        (d / f"{name}.txt").write_bytes(lr.taxonomy_file(nodes, names))
        made[name] = (tree, names, mr.node_markers(fps, cr.empty_of(s.o), seen, tree))
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    return s, d, made


@pytest.mark.parametrize("name", ["deep", "masked"])
def test_file_and_summary(work, name):
    s, d, made = work
    tree, names, nm = made[name]
    r = cli(["-i", "full.gz", "-a", "once.fa", "-T", f"{name}.txt", "-V", f"V_{name}.txt", "-o", "o.txt", "-t", "1"], d)
    want = mr.format_markers(nm, tree, names)
    assert want.count(b"\n") > 5
    assert (d / f"V_{name}.txt").read_bytes() == want
    assert line_of(r.stdout, b"markers: ") == [mr.summary_line(len(s.reads), nm, tree)]
    assert (d / "o.txt").read_bytes() == b""
    if name == "masked":
        assert int(nm[-1, 0]) > 0                                          # cells above every node, in the line


def test_beside_the_other_profiles(work):
    """-V beside -U -y -C -W: their files and lines are byte for byte those of a run without -V, and -V's are its own run's"""
    s, d, made = work
    tree, names, nm = made["deep"]
    others = ["-U", "U.txt", "-T", "deep.txt", "-y", "y.txt", "-C", "C.txt", "-W", "W.txt"]
    alone = cli(["-i", "full.gz", "-a", "once.fa", *others, "-o", "o.txt", "-t", "1"], d)
    kept = {f: (d / f).read_bytes() for f in ("U.txt", "y.txt", "C.txt", "W.txt")}
    assert all(kept.values())
    for f in kept:
        (d / f).unlink()
    both = cli(["-i", "full.gz", "-a", "once.fa", *others, "-V", "V_both.txt", "-o", "o.txt", "-t", "1"], d)
    for f, text in kept.items():
        assert (d / f).read_bytes() == text, f
    for head in (b"taxon cover: ", b"lca: ", b"cover: ", b"winners: "):
        assert line_of(both.stdout, head) == line_of(alone.stdout, head) and len(line_of(alone.stdout, head)) == 1
    assert line_of(alone.stdout, b"markers: ") == []
    assert (d / "V_both.txt").read_bytes() == mr.format_markers(nm, tree, names)
    assert line_of(both.stdout, b"markers: ") == [mr.summary_line(len(s.reads), nm, tree)]


def test_beside_the_gather_and_the_depth(work):
    """-G frees the table when nobody reads it after it: with -V it stays for the marker pass"""
    s, d, made = work
    tree, names, nm = made["deep"]
    alone = cli(["-i", "full.gz", "-a", "once.fa", "-G", "G.txt", "-D", "D.txt", "-o", "o.txt", "-t", "1"], d)
    kept = {f: (d / f).read_bytes() for f in ("G.txt", "D.txt")}
    both = cli(["-i", "full.gz", "-a", "once.fa", "-G", "G.txt", "-D", "D.txt", "-T", "deep.txt", "-V", "V_gather.txt", "-o", "o.txt", "-t", "1"], d)
    for f, text in kept.items():
        assert (d / f).read_bytes() == text, f
    assert line_of(both.stdout, b"gather: ") == line_of(alone.stdout, b"gather: ")
    assert (d / "V_gather.txt").read_bytes() == mr.format_markers(nm, tree, names)


def test_pairs_and_qualities_go_through(work):
    """-2 with mates shorter than k: every pair is its read alone; -q 0 over FASTQ records of the same reads cuts nothing: the
    file is the plain run's"""
    s, d, made = work
    tree, names, nm = made["deep"]
    r = cli(["-i", "full.gz", "-a", "once.fa", "-2", "short_mates.fa", "-T", "deep.txt", "-V", "V_pairs.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "V_pairs.txt").read_bytes() == mr.format_markers(nm, tree, names)
    assert line_of(r.stdout, b"markers: ") == [mr.summary_line(len(s.reads), nm, tree)]
    r = cli(["-i", "full.gz", "-a", "once.fq", "-q", "0", "-T", "deep.txt", "-V", "V_qual.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "V_qual.txt").read_bytes() == mr.format_markers(nm, tree, names)
    assert line_of(r.stdout, b"markers: ") == [mr.summary_line(len(s.reads), nm, tree)]


def test_an_id_beyond_the_index(work):
    s, d, _ = work
    (d / "beyond.txt").write_bytes(b"0 %d all\n0 1\n" % s.G)
    r = cli(["-i", "full.gz", "-a", "once.fa", "-T", "beyond.txt", "-V", "beyond_V.txt", "-o", "o_b.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-T: line 1 of beyond.txt: genome id %d is beyond the index's %d genomes" % (s.G, s.G) in r.stdout
    assert not (d / "beyond_V.txt").exists() and b"markers: " not in r.stdout
