"""`miekki -a <reads> -D <file>`: depth of coverage of the indexed genomes by a read set, alone and beside -P, -C and -W: the
reads are read and uploaded once, counted into the depth table over query_file's super-batches, and profiled in nine passes
over the matrix at the end.  The yardstick is the oracle's gated sketches and stored columns through tests/depth_ref.py: the
file's bytes and the stdout line are what its results format to, and the other files and lines are byte for byte those of a run
without -D."""

import pytest

import cover_ref as cr
import depth_ref as dr
import synth
import tally_ref as tr
from cli_util import cli, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records


def line_of(out, start):
    assert out.count(start) == 1
    at = out.index(start)
    return out[at:out.index(b"\n", at)]


class Want:
    """the file and the summary line of `times` copies of `reads`"""

    def __init__(self, o, fps, reads, times=1):
        h, fp_bits = o.number_minimizer_log2, o.number_bit_minimizer
        self.tab = dr.table(dr.mult(o, reads) * times)
        self.med, self.sum, self.cov = dr.profile(o, self.tab, fps)
        self.cells, self.sat = int((self.tab > 0).sum()), int((self.tab == 255).sum())
        self.file = dr.format_depth(self.med, self.sum, self.cov, o.sketch_size)
        self.line = dr.summary_line(len(reads) * times, self.cells, self.sat, h, fp_bits, self.cov)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the sample's genomes as files and as a dumped index, its reads as records (27 times over, with two records shorter
    than k among them)"""
    s = tr.Sample()
    d = tmp_path_factory.mktemp("depth")
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
    return s, d, base, cr.stored(s.o)


def test_depth_file_and_summary(work):
    s, d, base, fps = work
    w = Want(s.o, fps, s.reads, REPEATS)                                   # (the two short records are not counted; repeats DO count)
    assert w.sat > 0 and w.sat < w.cells and len(set(w.med.tolist())) >= 5 and (w.cov > 0).sum() > 1000
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-D", "dep.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "dep.txt").read_bytes() == w.file
    assert w.line + b"\n" in r.stdout
    assert b"profile:" not in r.stdout and b"cover:" not in r.stdout and b"winners:" not in r.stdout
    assert (d / "o.txt").read_bytes() == b""
    # the index built in the same run, fifty reads
    few = Want(s.o, fps, s.reads[:50])
    r = cli(["-l", "genomes.lst", "-a", "few.fa", "-D", "dep_l.txt", "-o", "o_l.txt", *base], d)
    assert (d / "dep_l.txt").read_bytes() == few.file
    assert few.line + b"\n" in r.stdout
    assert (d / "o_l.txt").read_bytes() == b""
    # one read of 300 bases: genomes without a covered fingerprint have no line
    one = Want(s.o, fps, s.reads[:1])
    assert 0 < (one.cov > 0).sum() < s.c.G
    (d / "one.fa").write_bytes(records(s.reads[:1]))
    r = cli(["-i", "full.gz", "-a", "one.fa", "-D", "dep_1.txt", "-o", "o_1.txt", "-t", "1"], d)
    assert (d / "dep_1.txt").read_bytes() == one.file
    assert one.line + b"\n" in r.stdout


def test_beside_profile_cover_and_winners(work):
    """-D with -P, -C and -W over two super-batches: the depth file is right, and the other three files and lines are byte for
    byte those of a run without -D"""
    s, d, base, fps = work
    w = Want(s.o, fps, s.reads, REPEATS)
    common = ["-i", "full.gz", "-a", "reads.fa", "-t", "1"]
    without = cli([*common, "-P", "prof_0.txt", "-C", "cov_0.txt", "-W", "win_0.txt", "-o", "o_0.txt"], d)
    beside = cli([*common, "-D", "dep_4.txt", "-P", "prof_4.txt", "-C", "cov_4.txt", "-W", "win_4.txt", "-o", "o_4.txt"], d)
    assert b"depth:" not in without.stdout
    assert (d / "dep_4.txt").read_bytes() == w.file
    assert line_of(beside.stdout, b"depth:") == w.line
    for name in ("prof", "cov", "win"):
        assert (d / f"{name}_0.txt").read_bytes() and (d / f"{name}_4.txt").read_bytes() == (d / f"{name}_0.txt").read_bytes()
    for tag in (b"profile:", b"cover:", b"winners:"):
        assert line_of(beside.stdout, tag) == line_of(without.stdout, tag)
    assert (d / "cov_0.txt").read_bytes() == cr.format_cover(w.cov, s.o.sketch_size)          # (depth's covered is the cover's)
    assert (d / "o_4.txt").read_bytes() == b""


@pytest.mark.parametrize("args,devices,env", [
    (["-i", "full.gz", "-D", "no.txt"], "0", None),                                       # without -a
    (["-i", "full.gz", "-a", "few.fa", "-D", "no.txt", "-e"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-D", "no.txt", "-A", "genomes.lst"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-D", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-D", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-D", "no.txt", "-n", "10"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-D", "no.txt", "-n", "0"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-D", "no.txt"], "0,0", None),                     # several GPUs in the process
    (["-l", "genomes.lst", "-a", "few.fa", "-D", "no.txt"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env):
    d = work[1]
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and b"-D" in r.stdout
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_depth_file_that_cannot_be_written(work):
    d = work[1]
    r = cli(["-i", "full.gz", "-a", "few.fa", "-D", "no_such_dir/dep.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-D: cannot write no_such_dir/dep.txt" in r.stdout
