"""`miekki -a <reads> -P <file>`: the profile of a read set, summed on the device over query_file's super-batches.  The
yardstick is the oracle's filter_results through tests/tally_ref.py: the file's bytes and the stdout line are what its
tally formats to."""
import gzip

import pytest

import synth
import tally_ref as tr
from cli_util import cli, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the sample's genomes as files and as a dumped index, its reads as records (27 times over, with two records shorter
    than k among them), and the oracle's tally of the reads at -s 20's thresholds"""
    s = tr.Sample()
    d = tmp_path_factory.mktemp("tally")
    for g, seq in enumerate(s.c.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.c.G)))
    k, h, fp_bits, b, threshold = s.c.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    once = records(s.reads)
    assert REPEATS * len(s.reads) > 16384
    short = b">short\n" + s.reads[0][:k - 1] + b"\n"
    (d / "reads.fa").write_bytes(short + once * REPEATS + short)
    (d / "reads.fa.gz").write_bytes(gzip.compress(short + once * REPEATS + short, 1))
    (d / "few.fa").write_bytes(records(s.reads[:50]))
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    return s, d, base, tr.tally(s.o, s.read_rows, 10, 0.5 * threshold)


def test_profile_file_and_summary(work):
    s, d, base, once = work
    want = once * REPEATS
    n = REPEATS * len(s.reads)                                             # (the two short records are not counted)
    assert (want[:, 0] > 0).sum() > 500 and want[:, 1].sum() == 0 and want[:, 2].sum() == n
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-P", "prof.txt", "-o", "o.txt", "-t", "1"], d)
    assert (d / "prof.txt").read_bytes() == tr.format_profile(want)
    assert tr.summary_line(want, n) + b"\n" in r.stdout
    assert (d / "o.txt").read_bytes() == b""
    # the gzip'd reads; and the index built in the same run
    r = cli(["-i", "full.gz", "-a", "reads.fa.gz", "-P", "prof_gz.txt", "-o", "o_gz.txt", "-t", "1"], d)
    assert (d / "prof_gz.txt").read_bytes() == tr.format_profile(want) and tr.summary_line(want, n) + b"\n" in r.stdout
    r = cli(["-l", "genomes.lst", "-a", "few.fa", "-P", "prof_l.txt", "-o", "o_l.txt", *base], d)
    few = tr.tally(s.o, s.read_rows[:50], 10, 0.5 * s.c.THRESHOLD)
    assert (d / "prof_l.txt").read_bytes() == tr.format_profile(few) and tr.summary_line(few, 50) + b"\n" in r.stdout
    assert (d / "o_l.txt").read_bytes() == b""


def test_profile_at_a_threshold_that_leaves_reads_unassigned(work):
    """-s 200: min_intersection 100 -- some reads list nothing, many list one genome only"""
    s, d, base, _ = work
    want = tr.tally(s.o, s.read_rows, 10, 100.0)
    assert 0 < want[:, 2].sum() < len(s.reads) and want[:, 1].sum() > 100
    args = [a if a != str(s.c.THRESHOLD) else "200" for a in base]
    assert args != base
    (d / "once.fa").write_bytes(records(s.reads))
    r = cli(["-l", "genomes.lst", "-a", "once.fa", "-P", "prof200.txt", "-o", "o200.txt", *args], d)
    assert (d / "prof200.txt").read_bytes() == tr.format_profile(want)
    assert tr.summary_line(want, len(s.reads)) + b"\n" in r.stdout


@pytest.mark.parametrize("args,devices,env", [
    (["-i", "full.gz", "-P", "no.txt"], "0", None),                                       # without -a
    (["-i", "full.gz", "-a", "few.fa", "-P", "no.txt", "-e"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-P", "no.txt", "-A", "genomes.lst"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-P", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-P", "no.txt", "-X"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-P", "no.txt", "-n", "10"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-P", "no.txt", "-n", "0"], "0", None),
    (["-i", "full.gz", "-a", "few.fa", "-P", "no.txt"], "0,0", None),                     # several GPUs in the process
    (["-l", "genomes.lst", "-a", "few.fa", "-P", "no.txt"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env):
    _, d, _, _ = work
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and b"-P" in r.stdout
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_profile_that_cannot_be_written(work):
    _, d, _, _ = work
    r = cli(["-i", "full.gz", "-a", "few.fa", "-P", "no_such_dir/prof.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-P: cannot write no_such_dir/prof.txt" in r.stdout
