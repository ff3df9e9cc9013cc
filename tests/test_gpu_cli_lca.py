"""`miekki -a <reads> -T <taxonomy> -y <report> [-Y <per read>] [-m <margin>]`: every read placed in a taxonomy by lowest
common ancestor on the device over query_file's super-batches.  The yardstick is the oracle's filter_results through
tests/lca_ref.py: the files' bytes and the stdout line are what its placement formats to."""
import os

import numpy as np
import pytest

import clade_ref as cr
import lca_ref as lr
import synth
from cli_util import cli, line_of, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the grouped collection as a dumped index, its reads as records (once, and 27 times over with two records shorter than
    k among them), the taxonomy files, and the oracle's lists of the reads at -s 20's thresholds"""
    s = lr.Grouped()
    d = tmp_path_factory.mktemp("lca")
    for g, seq in enumerate(s.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.G)))
    k, h, fp_bits, b, threshold = s.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    once = records(s.reads)
    short = b">short\n" + s.reads[0][:k - 1] + b"\n"
    (d / "reads.fa").write_bytes(short + once * REPEATS + short)
    (d / "once.fa").write_bytes(once)
    trees, names = {}, {}
    for name, nodes in lr.taxonomies(s.G).items():
        trees[name], names[name] = lr.Tree(nodes, s.G), lr.names_of(nodes)
        (d / f"{name}.txt").write_bytes(lr.taxonomy_file(nodes, names[name]))
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    return s, d, trees, names, cr.per_query(s.o, s.read_rows, 10, 0.5 * threshold)


def test_report_reads_and_summary(work):
    s, d, trees, names, lists = work
    n = REPEATS * len(s.reads)                                             # (the two short records are not counted)
    assert n > 16384
    # more than one super-batch: the counters accumulate, the ordinals of -Y go on
    t, per_read = lr.lca_tally(lists, trees["deep"], 10)
    want = t * np.uint64(REPEATS)
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-T", "deep.txt", "-y", "deep_y.txt", "-Y", "deep_Y.txt", "-m", "10", "-o", "o.txt", "-t", "1"], d)
    assert (d / "deep_y.txt").read_bytes() == lr.format_report(want, trees["deep"], names["deep"])
    assert (d / "deep_Y.txt").read_bytes() == lr.format_reads(np.tile(per_read, REPEATS))
    assert line_of(r.stdout, b"lca: ") == [lr.summary_line(want, n, 10)]
    assert (d / "o.txt").read_bytes() == b""
    assert len({int(v) for v in per_read}) > 8                             # (unassigned reads, `-`: the empty taxonomy below)


@pytest.mark.parametrize("name", ["flat", "deep", "masked", "single", "empty"])
def test_every_taxonomy_at_both_margins(work, name):
    """the reads once, at the default margin (100) and at 10; -Y is optional"""
    s, d, trees, names, lists = work
    for margin in (100, 10):
        t, per_read = lr.lca_tally(lists, trees[name], margin)
        args = ["-i", "full.gz", "-a", "once.fa", "-T", f"{name}.txt", "-y", f"{name}_y.txt", "-o", "o.txt", "-t", "1"]
        args += ["-m", "10", "-Y", f"{name}_each_Y.txt"] if margin == 10 else []
        r = cli(args, d)
        assert (d / f"{name}_y.txt").read_bytes() == lr.format_report(t, trees[name], names[name]), margin
        if margin == 10:
            assert (d / f"{name}_each_Y.txt").read_bytes() == lr.format_reads(per_read)
        else:
            assert not (d / f"{name}_each_Y.txt").exists()
        assert line_of(r.stdout, b"lca: ") == [lr.summary_line(t, len(s.reads), margin)]
    if name == "flat":
        assert lr.lca_tally(lists, trees["flat"], 10)[0][-1, 0] > 0 and b"\t*\n" in (d / "flat_each_Y.txt").read_bytes()   # above every node


def test_beside_the_other_profiles(work):
    """-T -y beside -P -p -C: their files and lines are byte for byte those of a run without -T"""
    s, d, trees, names, lists = work
    fine, _ = cr.clade_file(cr.layouts(s.G)["fine"])
    (d / "fine_clades.txt").write_bytes(fine)
    others = ["-P", "P.txt", "-L", "fine_clades.txt", "-p", "p.txt", "-C", "C.txt"]
    alone = cli(["-i", "full.gz", "-a", "once.fa", *others, "-o", "o.txt", "-t", "1"], d)
    kept = {f: (d / f).read_bytes() for f in ("P.txt", "p.txt", "C.txt")}
    assert all(kept.values())
    for f in kept:
        (d / f).unlink()
    both = cli(["-i", "full.gz", "-a", "once.fa", *others, "-T", "masked.txt", "-y", "y_both.txt", "-Y", "Y_both.txt", "-m", "0", "-o", "o.txt", "-t", "1"], d)
    for f, text in kept.items():
        assert (d / f).read_bytes() == text, f
    for head in (b"profile: ", b"clades: ", b"cover: "):
        assert line_of(both.stdout, head) == line_of(alone.stdout, head) and len(line_of(alone.stdout, head)) == 1
    assert line_of(alone.stdout, b"lca: ") == []
    t, per_read = lr.lca_tally(lists, trees["masked"], 0)
    assert (d / "y_both.txt").read_bytes() == lr.format_report(t, trees["masked"], names["masked"])
    assert (d / "Y_both.txt").read_bytes() == lr.format_reads(per_read)
    assert line_of(both.stdout, b"lca: ") == [lr.summary_line(t, len(s.reads), 0)]


def test_every_sink_in_one_run(work):
    """-P -L -p -T -y -Y -C -W -D -G at once: every file is byte for byte the one its flag writes in a run of its own, and
    the summary lines are those runs' lines, in the order profile, clades, lca, cover, winners, depth, gather.  (-G's own run
    has -D beside it: its picks carry a fifth field from the depth table where there is one.)"""
    s, d, _, _, _ = work
    fine, _ = cr.clade_file(cr.layouts(s.G)["fine"])
    (d / "all_clades.txt").write_bytes(fine)
    depth = ["-D", "{}D.txt"]
    sinks = ((b"profile: ", ["-P", "{}P.txt"], []), (b"clades: ", ["-L", "all_clades.txt", "-p", "{}p.txt"], []),
             (b"lca: ", ["-T", "deep.txt", "-y", "{}y.txt", "-Y", "{}Y.txt", "-m", "10"], []), (b"cover: ", ["-C", "{}C.txt"], []),
             (b"winners: ", ["-W", "{}W.txt"], []), (b"depth: ", depth, []), (b"gather: ", ["-G", "{}G.txt"], depth))

    def run(tag, flags, heads):
        """the files of `flags` by their names without the tag, and the lines that one of `heads` starts, in stdout's order"""
        r = cli(["-i", "full.gz", "-a", "once.fa", *(a.format(tag) for a in flags), "-o", "o.txt", "-t", "1"], d)
        files = {a.format(""): (d / a.format(tag)).read_bytes() for a in flags if a.startswith("{}")}
        return files, [l for l in (l.lstrip(b"-") for l in r.stdout.split(b"\n")) if any(l.startswith(h) for h in heads)]

    want_files, want_lines = {}, []
    for i, (head, flags, beside) in enumerate(sinks):
        files, lines = run(f"own{i}_", flags + beside, [head])
        own = {f: text for f, text in files.items() if f in {a.format("") for a in flags}}
        assert len(lines) == 1 and own and all(own.values()), head
        want_files.update(own)
        want_lines += lines
    files, lines = run("all_", [a for _, flags, _ in sinks for a in flags], [head for head, _, _ in sinks])
    assert sorted(files) == sorted(want_files) and len(files) == 8
    for f, text in want_files.items():
        assert files[f] == text, f
    assert lines == want_lines
    assert (d / "o.txt").read_bytes() == b""


def test_an_id_beyond_the_index(work):
    s, d, _, _, _ = work
    (d / "beyond.txt").write_bytes(b"0 %d all\n0 1\n" % s.G)
    r = cli(["-i", "full.gz", "-a", "once.fa", "-T", "beyond.txt", "-y", "beyond_y.txt", "-Y", "beyond_Y.txt", "-o", "o_b.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-T: line 1 of beyond.txt: genome id %d is beyond the index's %d genomes" % (s.G, s.G) in r.stdout
    assert not (d / "beyond_y.txt").exists() and not (d / "beyond_Y.txt").exists()
    assert b"lca: " not in r.stdout


def test_refusals_that_need_the_device_list(work):
    """several GPUs in the process, one process per GPU: -P's refusals, for -y"""
    _, d, _, _, _ = work
    for devices, env in (("0,0", None), ("0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"})):
        r = cli(["-i", "full.gz", "-a", "once.fa", "-T", "deep.txt", "-y", "no.txt", "-Y", "no_Y.txt", "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
        assert r.returncode == 1 and b"-y is not supported" in r.stdout and b"Using " not in r.stdout
        assert not (d / "no.txt").exists() and not (d / "no_Y.txt").exists() and not (d / "no_out.txt").exists()


def test_refusals_before_any_device(work):
    """what needs no device is refused with exit status 1 and nothing written, beside a real index as beside none"""
    _, d, _, _, _ = work
    (d / "overlap.txt").write_bytes(b"0 99\n10 19\n15 30\n")
    for args, says in ((["-y", "no.txt"], b"it needs -T"), (["-T", "deep.txt"], b"it needs -y"), (["-Y", "no_Y.txt"], b"it needs -T"),
                       (["-P", "no_P.txt", "-m", "10"], b"it needs -T"), (["-T", "deep.txt", "-y", "no.txt", "-m", "101"], b"-m takes a percentage"),
                       (["-T", "deep.txt", "-y", "no.txt", "-n", "5"], b"it takes no -n"), (["-T", "deep.txt", "-y", "no.txt", "-e"], b"-y"),
                       (["-T", "overlap.txt", "-y", "no.txt"], b"line 3 of overlap.txt"), (["-T", "nowhere.txt", "-y", "no.txt"], b"-T: cannot read nowhere.txt")):
        before = sorted(os.listdir(d))
        r = cli(["-i", "full.gz", "-a", "once.fa", *args, "-o", "no_out.txt"], d, ok=False)
        assert r.returncode == 1 and says in r.stdout and b"Using " not in r.stdout, r.stdout
        assert sorted(os.listdir(d)) == before


def test_a_report_that_cannot_be_written(work):
    _, d, _, _, _ = work
    r = cli(["-i", "full.gz", "-a", "once.fa", "-T", "deep.txt", "-y", "no_such_dir/y.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-y: cannot write no_such_dir/y.txt" in r.stdout
