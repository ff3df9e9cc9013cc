"""`miekki -a <reads> -G <file> [-g <int>]`: the greedy gather over the cover table of a read set, alone and beside -P, -C, -W and
-D: the reads are read and uploaded once, the table is marked once, and the rounds run at the end.  The yardstick is the
oracle's gated sketches and stored columns through tests/gather_ref.py: the file's bytes, in pick order, and the stdout line
are what its picks format to, and the other files and lines are byte for byte those of a run without -G."""
import os
import subprocess

import pytest

import cover_ref as cr
import depth_ref as dr
import gather_ref as gr
import synth
import tally_ref as tr
from cli_util import CLI, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records


def cli(args, cwd, devices="0", env=None, ok=True):
    e = dict(os.environ, MIEKKI_DEVICES=devices)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK", "MIEKKI_GATHER_ROUNDS", "MIEKKI_GATHER_RECOUNT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([CLI, *args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=e)
    if ok:
        assert r.returncode == 0, r.stdout.decode(errors="replace")
    return r


def line_of(out, start):
    assert out.count(start) == 1
    at = out.index(start)
    return out[at:out.index(b"\n", at)]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the sample's genomes as a dumped index, its reads as records (27 times over, with two records shorter than k among
    them), and the yardstick's picks at -g's default of 10 with the depth table of the 27 copies"""
    s = tr.Sample()
    d = tmp_path_factory.mktemp("gather")
    for g, seq in enumerate(s.c.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.c.G)))
    k, h, fp_bits, b, threshold = s.c.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    short = b">short\n" + s.reads[0][:k - 1] + b"\n"
    assert REPEATS * len(s.reads) > 16384
    (d / "reads.fa").write_bytes(short + records(s.reads) * REPEATS + short)
    (d / "few.fa").write_bytes(records(s.reads[:50]))
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    fps = cr.stored(s.o)
    table = dr.table(dr.mult(s.o, s.reads) * REPEATS)
    assert (table == 255).any()
    want = gr.gather(s.o, cr.seen(s.o, s.reads), fps, min_new=10, table=table)
    assert len(want[0]) > 100 and (want[0]["fresh"] >= 40).sum() > 20
    return s, d, base, fps, want


def test_gather_file_and_summary(work):
    s, d, base, fps, (picks, cells, explained) = work
    n = len(s.reads) * REPEATS                                             # (the two short records are not counted)
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-G", "gat.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "gat.txt").read_bytes() == gr.format_gather(picks)         # pick order, four fields
    assert gr.summary_line(n, explained, cells, len(picks), 10) + b"\n" in r.stdout
    assert all(tag not in r.stdout for tag in (b"profile:", b"cover:", b"winners:", b"depth:"))
    assert (d / "o.txt").read_bytes() == b""
    # -g 40: the prefix of the picks with at least 40 new cells
    at40 = picks[picks["fresh"] >= 40]
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-G", "gat_40.txt", "-g", "40", "-o", "o_40.txt", "-t", "1"], d)
    assert 0 < len(at40) < len(picks) and (d / "gat_40.txt").read_bytes() == gr.format_gather(at40)
    assert gr.format_gather(picks).startswith(gr.format_gather(at40))
    assert gr.summary_line(n, int(at40["fresh"].sum()), cells, len(at40), 40) + b"\n" in r.stdout
    # the index built in the same run, fifty reads, one round queued per host wait
    few = gr.gather(s.o, cr.seen(s.o, s.reads[:50]), fps, min_new=10)
    assert 0 < len(few[0]) < len(picks)
    r = cli(["-l", "genomes.lst", "-a", "few.fa", "-G", "gat_l.txt", "-o", "o_l.txt", *base], d, env={"MIEKKI_GATHER_ROUNDS": "1"})
    assert (d / "gat_l.txt").read_bytes() == gr.format_gather(few[0])
    assert gr.summary_line(50, few[2], few[1], len(few[0]), 10) + b"\n" in r.stdout
    assert (d / "o_l.txt").read_bytes() == b""


def test_beside_profile_cover_winners_and_depth(work):
    """-G with -P, -C, -W and -D over two super-batches: the gather file is right and has its fifth field, and the other four
    files and lines are byte for byte those of a run without -G"""
    s, d, base, fps, (picks, cells, explained) = work
    common = ["-i", "full.gz", "-a", "reads.fa", "-t", "1"]
    without = cli([*common, "-P", "prof_0.txt", "-C", "cov_0.txt", "-W", "win_0.txt", "-D", "dep_0.txt", "-o", "o_0.txt"], d)
    beside = cli([*common, "-G", "gat_5.txt", "-P", "prof_5.txt", "-C", "cov_5.txt", "-W", "win_5.txt", "-D", "dep_5.txt", "-o", "o_5.txt"], d)
    assert b"gather:" not in without.stdout
    assert picks["depth_sum"].min() > 0
    assert (d / "gat_5.txt").read_bytes() == gr.format_gather(picks, True)
    assert line_of(beside.stdout, b"gather:") == gr.summary_line(len(s.reads) * REPEATS, explained, cells, len(picks), 10)
    for name in ("prof", "cov", "win", "dep"):
        assert (d / f"{name}_0.txt").read_bytes() and (d / f"{name}_5.txt").read_bytes() == (d / f"{name}_0.txt").read_bytes()
    for tag in (b"profile:", b"cover:", b"winners:", b"depth:"):
        assert line_of(beside.stdout, tag) == line_of(without.stdout, tag)
    assert (d / "o_5.txt").read_bytes() == b""
    # beside -C alone there is no depth table: four fields
    cli([*common, "-G", "gat_c.txt", "-C", "cov_c.txt", "-o", "o_c.txt"], d)
    assert (d / "gat_c.txt").read_bytes() == gr.format_gather(picks)
    assert (d / "cov_c.txt").read_bytes() == (d / "cov_0.txt").read_bytes()


@pytest.mark.parametrize("args,devices,env,flag", [
    (["-i", "full.gz", "-G", "no.txt"], "0", None, b"-G"),                                 # without -a
    (["-i", "full.gz", "-a", "few.fa", "-G", "no.txt", "-e"], "0", None, b"-G"),
    (["-i", "full.gz", "-a", "few.fa", "-G", "no.txt", "-A", "genomes.lst"], "0", None, b"-G"),
    (["-i", "full.gz", "-a", "few.fa", "-G", "no.txt", "-X"], "0", None, b"-G"),
    (["-i", "full.gz", "-G", "no.txt", "-X"], "0", None, b"-G"),
    (["-i", "full.gz", "-a", "few.fa", "-G", "no.txt", "-n", "10"], "0", None, b"-G"),
    (["-i", "full.gz", "-a", "few.fa", "-G", "no.txt", "-n", "0"], "0", None, b"-G"),
    (["-i", "full.gz", "-a", "few.fa", "-G", "no.txt"], "0,0", None, b"-G"),               # several GPUs in the process
    (["-l", "genomes.lst", "-a", "few.fa", "-G", "no.txt"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}, b"-G"),
    (["-i", "full.gz", "-a", "few.fa", "-G", "no.txt", "-g", "0"], "0", None, b"-g"),
    (["-i", "full.gz", "-a", "few.fa", "-g", "5"], "0", None, b"-g"),                      # -g without -G
    (["-i", "full.gz", "-a", "few.fa", "-C", "no.txt", "-g", "5"], "0", None, b"-g"),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env, flag):
    d = work[1]
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and flag in r.stdout
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_gather_file_that_cannot_be_written(work):
    d = work[1]
    r = cli(["-i", "full.gz", "-a", "few.fa", "-G", "no_such_dir/gat.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-G: cannot write no_such_dir/gat.txt" in r.stdout
