"""`miekki -a <reads> -C <file>`: breadth of coverage of the indexed genomes by a read set, marked on the device over
query_file's super-batches and counted in one pass over the matrix.  The yardstick is the oracle's gated sketches and stored
columns through tests/cover_ref.py: the file's bytes and the stdout line are what its counts format to."""

import pytest

import cover_ref as cr
import synth
import tally_ref as tr
from cli_util import cli, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the sample's genomes as files and as a dumped index, its reads as records (27 times over, with two records shorter
    than k among them), and the oracle's cover of the reads"""
    s = tr.Sample()
    d = tmp_path_factory.mktemp("cover")
    for g, seq in enumerate(s.c.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.c.G)))
    k, h, fp_bits, b, threshold = s.c.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    once = records(s.reads)
    assert REPEATS * len(s.reads) > 16384
    short = b">short\n" + s.reads[0][:k - 1] + b"\n"
    (d / "reads.fa").write_bytes(short + once * REPEATS + short)
    (d / "few.fa").write_bytes(records(s.reads[:50]))
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    fps = cr.stored(s.o)
    seen = cr.seen(s.o, s.reads)
    return s, d, base, fps, cr.covered(s.o, seen, fps), int(seen.sum())


def test_cover_file_and_summary(work):
    s, d, base, fps, cov, cells = work
    k, h, fp_bits, b, threshold = s.c.par
    n = REPEATS * len(s.reads)                                             # (the two short records are not counted; repeats mark nothing new)
    assert (cov > 0).sum() > 1000
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-C", "cov.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "cov.txt").read_bytes() == cr.format_cover(cov, s.o.sketch_size)
    assert cr.summary_line(n, cells, h, fp_bits, cov) + b"\n" in r.stdout
    assert b"profile:" not in r.stdout
    assert (d / "o.txt").read_bytes() == b""
    # the index built in the same run
    seen = cr.seen(s.o, s.reads[:50])
    few = cr.covered(s.o, seen, fps)
    r = cli(["-l", "genomes.lst", "-a", "few.fa", "-C", "cov_l.txt", "-o", "o_l.txt", *base], d)
    assert (d / "cov_l.txt").read_bytes() == cr.format_cover(few, s.o.sketch_size)
    assert cr.summary_line(50, int(seen.sum()), h, fp_bits, few) + b"\n" in r.stdout
    assert (d / "o_l.txt").read_bytes() == b""
    # one read of 300 bases: genomes without a covered fingerprint have no line (fifty reads already cover every genome
    # of this 8-bit index by chance)
    seen = cr.seen(s.o, s.reads[:1])
    one = cr.covered(s.o, seen, fps)
    assert 0 < (one > 0).sum() < s.c.G
    (d / "one.fa").write_bytes(records(s.reads[:1]))
    r = cli(["-i", "full.gz", "-a", "one.fa", "-C", "cov_1.txt", "-o", "o_1.txt", "-t", "1"], d)
    assert (d / "cov_1.txt").read_bytes() == cr.format_cover(one, s.o.sketch_size)
    assert cr.summary_line(1, int(seen.sum()), h, fp_bits, one) + b"\n" in r.stdout


def profile_line(out):
    assert out.count(b"profile:") == 1
    at = out.index(b"profile:")
    return out[at:out.index(b"\n", at)]


def test_profile_and_cover_together(work):
    """-P and -C in one run: both files are right, and -P's file and line are byte for byte those of a run without -C"""
    s, d, base, fps, cov, cells = work
    k, h, fp_bits, b, threshold = s.c.par
    n = REPEATS * len(s.reads)
    alone = cli(["-i", "full.gz", "-a", "reads.fa", "-P", "prof_alone.txt", "-o", "o_a.txt", "-t", "1"], d)
    both = cli(["-i", "full.gz", "-a", "reads.fa", "-P", "prof_both.txt", "-C", "cov_both.txt", "-o", "o_b.txt", "-t", "1"], d)
    want = tr.tally(s.o, s.read_rows, 10, 0.5 * threshold) * REPEATS
    assert (d / "prof_alone.txt").read_bytes() == tr.format_profile(want)
    assert (d / "prof_both.txt").read_bytes() == (d / "prof_alone.txt").read_bytes()
    line = profile_line(alone.stdout)                                      # (it follows the progress marks on their line)
    assert line == tr.summary_line(want, n) and line == profile_line(both.stdout)
    assert b"cover:" not in alone.stdout
    assert (d / "cov_both.txt").read_bytes() == cr.format_cover(cov, s.o.sketch_size)
    assert cr.summary_line(n, cells, h, fp_bits, cov) + b"\n" in both.stdout
    assert (d / "o_b.txt").read_bytes() == b""


@pytest.mark.parametrize("args,devices,env", [
    (["-i", "full.gz", "-C", "no.txt"], "0", None),                                       # without -a
    (["-i", "full.gz", "-a", "few.fa", "-C", "no.txt", "-e"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-C", "no.txt", "-A", "genomes.lst"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-C", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-C", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-C", "no.txt", "-n", "10"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-C", "no.txt", "-n", "0"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-C", "no.txt"], "0,0", None),                     # several GPUs in the process
    (["-l", "genomes.lst", "-a", "few.fa", "-C", "no.txt"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env):
    d = work[1]
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and b"-C" in r.stdout
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_cover_file_that_cannot_be_written(work):
    d = work[1]
    r = cli(["-i", "full.gz", "-a", "few.fa", "-C", "no_such_dir/cov.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-C: cannot write no_such_dir/cov.txt" in r.stdout
