"""`miekki -a <reads> -W <file>`: the winner-takes-all screen of the indexed genomes by a read set, alone and beside -C and -P:
the reads are read, uploaded and marked once, and with -C one count pass serves both files.  The yardsticks are the oracle's
through tests/winners_ref.py, tests/cover_ref.py and tests/tally_ref.py: the files' bytes and the stdout lines are what their
counts format to, and -C's and -P's are byte for byte those of a run without -W."""

import pytest

import cover_ref as cr
import synth
import tally_ref as tr
import winners_ref as wr
from cli_util import cli, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records


def line_of(out, start):
    assert out.count(start) == 1
    at = out.index(start)
    return out[at:out.index(b"\n", at)]


class Want:
    def __init__(self, o, fps, reads):
        self.seen = cr.seen(o, reads)
        self.cells = int(self.seen.sum())
        self.cov = cr.covered(o, self.seen, fps)
        self.order = wr.order(self.cov, o.sketch_size)
        self.won, self.claimed = wr.won(o, self.seen, fps, self.order)
        self.file = wr.format_winners(self.won, self.cov, o.sketch_size)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the sample's genomes as a dumped index, its reads as records (27 times over, with two records shorter than k among
    them), and the oracle's screen of the reads"""
    s = tr.Sample()
    d = tmp_path_factory.mktemp("winners")
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
    return s, d, base, fps, Want(s.o, fps, s.reads)


def test_winners_file_and_summary(work):
    s, d, base, fps, w = work
    n = REPEATS * len(s.reads)                                             # (the two short records are not counted; repeats mark nothing new)
    assert 0 < (w.won > 0).sum() < (w.cov > 0).sum()
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-W", "win.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "win.txt").read_bytes() == w.file
    assert wr.summary_line(n, w.claimed, w.cells, w.won) + b"\n" in r.stdout
    assert b"profile:" not in r.stdout and b"cover:" not in r.stdout
    assert (d / "o.txt").read_bytes() == b""
    # the index built in the same run, fifty reads
    few = Want(s.o, fps, s.reads[:50])
    r = cli(["-l", "genomes.lst", "-a", "few.fa", "-W", "win_l.txt", "-o", "o_l.txt", *base], d)
    assert (d / "win_l.txt").read_bytes() == few.file
    assert wr.summary_line(50, few.claimed, few.cells, few.won) + b"\n" in r.stdout
    assert (d / "o_l.txt").read_bytes() == b""


def test_beside_cover_and_profile(work):
    """-W with -C, and with -C and -P, over two super-batches: every file is right, and -C's and -P's files and lines are byte
    for byte those of a run without -W"""
    s, d, base, fps, w = work
    k, h, fp_bits, b, threshold = s.c.par
    n = REPEATS * len(s.reads)
    common = ["-i", "full.gz", "-a", "reads.fa", "-t", "1"]
    without = cli([*common, "-C", "cov_0.txt", "-P", "prof_0.txt", "-o", "o_0.txt"], d)
    two = cli([*common, "-C", "cov_2.txt", "-W", "win_2.txt", "-o", "o_2.txt"], d)
    three = cli([*common, "-W", "win_3.txt", "-P", "prof_3.txt", "-C", "cov_3.txt", "-o", "o_3.txt"], d)
    tally = tr.tally(s.o, s.read_rows, 10, 0.5 * threshold) * REPEATS
    assert (d / "cov_0.txt").read_bytes() == cr.format_cover(w.cov, s.o.sketch_size)
    assert (d / "prof_0.txt").read_bytes() == tr.format_profile(tally)
    cover_line, profile_line = cr.summary_line(n, w.cells, h, fp_bits, w.cov), tr.summary_line(tally, n)
    assert line_of(without.stdout, b"cover:") == cover_line and line_of(without.stdout, b"profile:") == profile_line
    assert b"winners:" not in without.stdout
    for run, tag in ((two, "2"), (three, "3")):
        assert (d / f"win_{tag}.txt").read_bytes() == w.file
        assert (d / f"cov_{tag}.txt").read_bytes() == (d / "cov_0.txt").read_bytes()
        assert line_of(run.stdout, b"cover:") == cover_line
        assert line_of(run.stdout, b"winners:") == wr.summary_line(n, w.claimed, w.cells, w.won)
        assert (d / f"o_{tag}.txt").read_bytes() == b""
    assert b"profile:" not in two.stdout
    assert (d / "prof_3.txt").read_bytes() == (d / "prof_0.txt").read_bytes()
    assert line_of(three.stdout, b"profile:") == profile_line


@pytest.mark.parametrize("args,devices,env", [
    (["-i", "full.gz", "-W", "no.txt"], "0", None),                                       # without -a
    (["-i", "full.gz", "-a", "few.fa", "-W", "no.txt", "-e"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-W", "no.txt", "-A", "genomes.lst"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-W", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-W", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-W", "no.txt", "-n", "10"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-W", "no.txt", "-n", "0"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-W", "no.txt"], "0,0", None),                     # several GPUs in the process
    (["-l", "genomes.lst", "-a", "few.fa", "-W", "no.txt"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env):
    d = work[1]
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and b"-W" in r.stdout
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_winners_file_that_cannot_be_written(work):
    d = work[1]
    r = cli(["-i", "full.gz", "-a", "few.fa", "-W", "no_such_dir/win.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-W: cannot write no_such_dir/win.txt" in r.stdout
