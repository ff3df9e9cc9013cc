"""`miekki -a <reads> -L <clades> -p <file>`: the profile of a read set by clade, summed on the device over query_file's
super-batches.  The yardstick is the oracle's filter_results through tests/clade_ref.py: the file's bytes and the stdout line
are what its clade tally formats to."""

import numpy as np
import pytest

import clade_ref as cr
import synth
import tally_ref as tr
from cli_util import cli, line_of, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the sample's genomes as a dumped index, its reads as records (once, and 27 times over with two records shorter than k
    among them), the clade files of the layouts, and the oracle's lists of the reads at -s 20's thresholds"""
    s = tr.Sample()
    d = tmp_path_factory.mktemp("clades")
    for g, seq in enumerate(s.c.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.c.G)))
    k, h, fp_bits, b, threshold = s.c.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    once = records(s.reads)
    short = b">short\n" + s.reads[0][:k - 1] + b"\n"
    (d / "reads.fa").write_bytes(short + once * REPEATS + short)
    (d / "once.fa").write_bytes(once)
    maps = {}
    for name, clade in cr.layouts(s.c.G).items():
        text, maps[name] = cr.clade_file(clade)
        (d / f"{name}.txt").write_bytes(text)
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    return s, d, maps, cr.per_query(s.o, s.read_rows, 10, 0.5 * threshold)


def test_clade_profile_file_and_summary(work):
    s, d, maps, lists = work
    n = REPEATS * len(s.reads)                                             # (the two short records are not counted)
    assert n > 16384
    want = cr.clade_tally(lists, maps["fine"]) * np.uint64(REPEATS)
    assert (want[:, 0] > 0).all() and want[:, 2].sum() == n
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-L", "fine.txt", "-p", "fine_prof.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "fine_prof.txt").read_bytes() == cr.format_clade_profile(want, maps["fine"])
    assert cr.summary_line(want, n) + b"\n" in r.stdout
    assert (d / "o.txt").read_bytes() == b""
    # left-out genomes (the file does not name them); the other layouts on the reads once
    for name in ("masked", "single", "one", "coarse"):
        want = cr.clade_tally(lists, maps[name])
        r = cli(["-i", "full.gz", "-a", "once.fa", "-L", f"{name}.txt", "-p", f"{name}_prof.txt", "-o", "o.txt", "-t", "1"], d)
        assert (d / f"{name}_prof.txt").read_bytes() == cr.format_clade_profile(want, maps[name]), name
        assert cr.summary_line(want, len(s.reads)) + b"\n" in r.stdout
    assert cr.n_clades(maps["masked"]) == 10 and maps["masked"][1024] is None


def test_beside_the_other_profiles_one_scan(work):
    """-P -p: -P's file and line are byte for byte those of a run without -p; the same for -C"""
    s, d, maps, lists = work
    alone = cli(["-i", "full.gz", "-a", "once.fa", "-P", "P_alone.txt", "-C", "C_alone.txt", "-o", "o.txt", "-t", "1"], d)
    both = cli(["-i", "full.gz", "-a", "once.fa", "-P", "P_both.txt", "-C", "C_both.txt", "-L", "masked.txt", "-p", "p_both.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "P_both.txt").read_bytes() == (d / "P_alone.txt").read_bytes() != b""
    assert (d / "C_both.txt").read_bytes() == (d / "C_alone.txt").read_bytes() != b""
    for head in (b"profile: ", b"cover: "):
        assert line_of(both.stdout, head) == line_of(alone.stdout, head) and len(line_of(alone.stdout, head)) == 1
    want = cr.clade_tally(lists, maps["masked"])
    assert (d / "p_both.txt").read_bytes() == cr.format_clade_profile(want, maps["masked"])
    assert line_of(both.stdout, b"clades: ") == [cr.summary_line(want, len(s.reads))]
    assert (d / "P_alone.txt").read_bytes() == tr.format_profile(cr.plain_tally(lists, s.c.G))


def test_families_grouped_and_profiled(work):
    """-F, -K with that file, -F again on the grouped index: a file -L takes as it is, and every family is one line of -p.
    No read of the sample has two best genomes (test_gpu_tally.test_sample_preconditions_from_the_oracle_alone), so the
    counters do not depend on the order of the ids: they are the oracle's, by family."""
    s, d, maps, lists = work
    cli(["-i", "full.gz", "-F", "fam.txt", "-o", "o.txt", "-t", "1"], d)
    cli(["-i", "full.gz", "-K", "fam.txt", "-F", "fam_grouped.txt", "-d", "grouped.gz", "-o", "o.txt", "-t", "1"], d)
    order = [int(x) for x in (d / "fam.txt").read_bytes().split()]         # new id j is old id order[j]
    grouped = (d / "fam_grouped.txt").read_bytes()
    assert [int(x) for x in grouped.split()] == list(range(s.c.G))
    blocks = [[int(x) for x in blk.split()] for blk in grouped.split(b"\n\n")]
    assert len(blocks) < s.c.G and max(len(b) for b in blocks) >= 4          # (the planted species)
    new_clade = [c for c, blk in enumerate(blocks) for _ in blk]
    old_clade = [None] * s.c.G
    for j, g in enumerate(order):
        old_clade[g] = new_clade[j]
    want = cr.clade_tally(lists, old_clade)
    r = cli(["-i", "grouped.gz", "-a", "once.fa", "-L", "fam_grouped.txt", "-p", "fam_prof.txt", "-o", "o.txt", "-t", "1"], d)
    got = (d / "fam_prof.txt").read_bytes()
    assert got == cr.format_clade_profile(want, new_clade)
    assert cr.summary_line(want, len(s.reads)) + b"\n" in r.stdout
    rows = [[int(x) for x in l.split(b"\t")] for l in got.splitlines()]
    assert [r[0] for r in rows] == sorted({r[0] for r in rows})             # a family is one line
    assert all(blocks[r[0]][0] == r[1] and len(blocks[r[0]]) == r[2] for r in rows)
    # ... and the same in one run from the ungrouped file: -K first, -L's ids are those the queries see
    r = cli(["-i", "full.gz", "-K", "fam.txt", "-a", "once.fa", "-L", "fam_grouped.txt", "-p", "fam_prof2.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "fam_prof2.txt").read_bytes() == got


def test_an_id_beyond_the_index(work):
    s, d, _, _ = work
    (d / "beyond.txt").write_bytes(b"0\n1\n\n%d\n" % s.c.G)
    r = cli(["-i", "full.gz", "-a", "once.fa", "-L", "beyond.txt", "-p", "beyond_prof.txt", "-o", "o_b.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-L: genome id %d is beyond the index's %d genomes" % (s.c.G, s.c.G) in r.stdout
    assert not (d / "beyond_prof.txt").exists()
    assert b"clades: " not in r.stdout


def test_refusals_that_need_the_device_list(work):
    """several GPUs in the process, one process per GPU: -P's refusals, for -p"""
    _, d, _, _ = work
    for devices, env in (("0,0", None), ("0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"})):
        r = cli(["-i", "full.gz", "-a", "once.fa", "-L", "fine.txt", "-p", "no.txt", "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
        assert r.returncode == 1 and b"-p is not supported" in r.stdout and b"Using " not in r.stdout
        assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_profile_that_cannot_be_written(work):
    _, d, _, _ = work
    r = cli(["-i", "full.gz", "-a", "once.fa", "-L", "fine.txt", "-p", "no_such_dir/prof.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-p: cannot write no_such_dir/prof.txt" in r.stdout
