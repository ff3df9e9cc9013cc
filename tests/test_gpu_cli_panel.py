"""`miekki -S <list> -c <file>`: the cover of a cohort of read files, eight samples per table and pass over the matrix.  The
yardstick is the oracle's gated sketches and stored columns through tests/panel_ref.py: the file's bytes and the stdout lines
are what its counts format to, and a sample's lines without their first field are the -C file of a run with -a on its file."""

import pytest

import cover_ref as cr
import panel_ref as pr
import synth
import tally_ref as tr
from cli_util import cli, records

pytestmark = pytest.mark.gpu
BIG = 6                            # the sample whose file holds more than one super-batch of 16,384 records
REPEATS = 75


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the sample's genomes as files and as a dumped index; ten read files -- tr.Sample's queries dealt into eight (one without
    a record, one 75 times over with two records shorter than k among them: more than one super-batch) and two more -- and
    the oracle's cover of each"""
    s = tr.Sample()
    d = tmp_path_factory.mktemp("panel")
    for g, seq in enumerate(s.c.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.c.G)))
    k, h, fp_bits, b, threshold = s.c.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    dealt = pr.deal(s)
    dealt += [dealt[0][:5], dealt[4][:20]]
    assert len(dealt) == 10 and not dealt[2] and REPEATS * len(dealt[BIG]) > 16384
    short = b">short\n" + s.reads[0][:k - 1] + b"\n"
    counts = []
    for i, q in enumerate(dealt):
        text = short + records(q) * REPEATS + short if i == BIG else records(q)
        (d / f"sample{i}.fa").write_bytes(text)
        counts.append(len(q) * (REPEATS if i == BIG else 1))               # (the short records are not counted; repeats mark nothing new)
    (d / "samples.lst").write_bytes(b"".join(b"sample%d.fa\n" % i for i in range(10)) + b"\nx\n")      # (lines of up to 3 characters do not count)
    (d / "three.lst").write_bytes(b"sample3.fa\nsample2.fa\nsample8.fa\n")
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    fps = cr.stored(s.o)
    seens = pr.seen_per_sample(s.o, dealt)
    return s, d, base, counts, pr.covered(s.o, seens, fps), pr.cells(seens)


def test_panel_file_and_lines(work):
    s, d, base, counts, cov, cells = work
    k, h, fp_bits, b, threshold = s.c.par
    r = cli(["-i", "full.gz", "-S", "samples.lst", "-c", "panel.txt", "-o", "o.txt", "-t", "1"], d)
    got = (d / "panel.txt").read_bytes()
    assert got == pr.format_panel(cov, s.o.sketch_size)
    for i in range(10):
        assert pr.sample_line(i, counts[i], cells[i], h, fp_bits, cov[i]) + b"\n" in r.stdout
    assert pr.summary_line(10) + b"\n" in r.stdout and r.stdout.count(b"panel[") == 10 and r.stdout.count(b"panel: ") == 1
    assert r.stdout.index(b"panel[7]:") < r.stdout.index(b"panel[8]:") < r.stdout.index(b"panel[9]:") < r.stdout.index(b"panel:")
    assert b"cover:" not in r.stdout and (d / "o.txt").read_bytes() == b""
    # a sample's lines without the first field are the -C file of a run with -a on its file
    for i in (BIG, 8):
        cli(["-i", "full.gz", "-a", f"sample{i}.fa", "-C", f"cov{i}.txt", "-o", f"o{i}.txt", "-t", "1"], d)
        mine = b"".join(l.split(b"\t", 1)[1] for l in got.splitlines(True) if l.startswith(b"%d\t" % i))
        assert mine == (d / f"cov{i}.txt").read_bytes() == cr.format_cover(cov[i], s.o.sketch_size) and mine


def test_index_built_in_the_same_run(work):
    """-l ... -S ... -c: three samples in another order, the one without a record among them"""
    s, d, base, counts, cov, cells = work
    k, h, fp_bits, b, threshold = s.c.par
    r = cli(["-l", "genomes.lst", "-S", "three.lst", "-c", "panel_l.txt", "-o", "o_l.txt", *base], d)
    order = [3, 2, 8]
    assert (d / "panel_l.txt").read_bytes() == pr.format_panel(cov[order], s.o.sketch_size)
    for at, i in enumerate(order):
        assert pr.sample_line(at, counts[i], cells[i], h, fp_bits, cov[i]) + b"\n" in r.stdout
    assert pr.summary_line(3) + b"\n" in r.stdout
    assert (d / "o_l.txt").read_bytes() == b""


@pytest.mark.parametrize("args,devices,env,names", [
    (["-i", "full.gz", "-S", "samples.lst"], "0", None, b"-c"),                            # one flag without the other
    (["-i", "full.gz", "-c", "no.txt"], "0", None, b"-S"),
    (["-i", "full.gz", "-S", "no_such.lst", "-c", "no.txt"], "0", None, b"no_such.lst"),   # a list that cannot be read
    (["-i", "full.gz", "-S", "none.lst", "-c", "no.txt"], "0", None, b"none.lst"),         # ... or names no file
    (["-i", "full.gz", "-S", "gone.lst", "-c", "no.txt"], "0", None, b"sample 1 of gone.lst: gone.fa"),
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt", "-a", "sample0.fa"], "0", None, b"-a"),
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt", "-A", "genomes.lst"], "0", None, b"-A"),
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt", "-e"], "0", None, b"-e"),
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt", "-X"], "0", None, b"-X"),
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt", "-n", "10"], "0", None, b"-n"),
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt", "-a", "sample0.fa", "-C", "no_c.txt"], "0", None, b"-a"),
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt", "-C", "no_c.txt"], "0", None, b"-C"),      # -C needs -a
    (["-i", "full.gz", "-S", "samples.lst", "-c", "no.txt"], "0,0", None, b"several GPUs"),
    (["-l", "genomes.lst", "-S", "samples.lst", "-c", "no.txt"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}, b"one process per GPU"),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env, names):
    d = work[1]
    (d / "none.lst").write_bytes(b"\nab\n\nabc\n")
    (d / "gone.lst").write_bytes(b"sample0.fa\ngone.fa\n")
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and names in r.stdout and (b"-S" in r.stdout or b"-c" in r.stdout or b"-C" in r.stdout)
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists() and not (d / "no_c.txt").exists()


def test_a_panel_file_that_cannot_be_written(work):
    d = work[1]
    r = cli(["-i", "full.gz", "-S", "three.lst", "-c", "no_such_dir/panel.txt", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-c: cannot write no_such_dir/panel.txt" in r.stdout
