"""`miekki -a <reads> -E <file> [-I <rounds>] [-w <margin>]`: abundance by expectation-maximisation over the reads that
several genomes share, collected on the device over query_file's super-batches.  The yardstick is the oracle's filter_results
through tests/share_ref.py: the file's bytes and the stdout line are what its pool and rounds format to."""
import pytest

import clade_ref as cr
import lca_ref as lr
import pairs_ref as pr
import share_ref as sr
import synth
from cli_util import cli, line_of, records

pytestmark = pytest.mark.gpu
REPEATS = 27                       # 27 x 620 reads: more than one super-batch of 16,384 records
PAIRS = 120


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the grouped collection as a dumped index, its reads as records (once, and 27 times over with two records shorter than
    k among them), and the oracle's lists of the reads at -s 20's thresholds"""
    s = lr.Grouped()
    d = tmp_path_factory.mktemp("abundance")
    for g, seq in enumerate(s.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(s.G)))
    k, h, fp_bits, b, threshold = s.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    once = records(s.reads)
    short = b">short\n" + s.reads[0][:k - 1] + b"\n"
    (d / "reads.fa").write_bytes(short + once * REPEATS + short)
    (d / "once.fa").write_bytes(once)
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    return s, d, cr.per_query(s.o, s.read_rows, 10, 0.5 * threshold)


def wanted(lists, G, margin, R):
    """(the file, the line) of the queries whose lists are `lists`"""
    pool = sr.pool_of(lists, margin, G)
    A, delta, _, _ = sr.rounds(pool, R)
    return sr.format_abundance(A, pool.unique, pool.shared), sr.summary_line(pool, R, margin, delta)


def test_file_and_line(work):
    """the defaults one at a time: 50 rounds at -w 10, margin 100 at -I 7"""
    s, d, lists = work
    for flags, margin, R in ((["-w", "10"], 10, 50), (["-I", "7"], 100, 7), (["-I", "1", "-w", "0"], 0, 1)):
        text, line = wanted(lists, s.G, margin, R)
        assert text.count(b"\n") > 100
        r = cli(["-i", "full.gz", "-a", "once.fa", "-E", "E.txt", *flags, "-o", "o.txt", "-t", "1"], d)
        assert (d / "E.txt").read_bytes() == text, flags
        assert line_of(r.stdout, b"abundance: ") == [line]
        assert (d / "o.txt").read_bytes() == b""
        (d / "E.txt").unlink()
    assert len(sr.pool_of(lists, 100, s.G).lists) > 600 and sr.pool_of(lists, 10, s.G).settled > 400   # (shared reads; settled ones)


def test_more_than_one_super_batch(work):
    """27 x 620 reads and two records shorter than k: the pool fills batch by batch, -I 7 -w 10"""
    s, d, lists = work
    n = REPEATS * len(s.reads)
    assert n > 16384
    text, line = wanted(lists * REPEATS, s.G, 10, 7)
    r = cli(["-i", "full.gz", "-a", "reads.fa", "-E", "E_many.txt", "-I", "7", "-w", "10", "-o", "o.txt", "-t", "1"], d)
    assert (d / "E_many.txt").read_bytes() == text
    assert line_of(r.stdout, b"abundance: ") == [line] and line.startswith(b"abundance: %d queries, " % n)
    assert (d / "o.txt").read_bytes() == b""


def test_beside_the_other_profiles(work):
    """-E beside -P -C: their files and lines are byte for byte those of a run without -E"""
    s, d, lists = work
    others = ["-P", "P.txt", "-C", "C.txt"]
    alone = cli(["-i", "full.gz", "-a", "once.fa", *others, "-o", "o.txt", "-t", "1"], d)
    kept = {f: (d / f).read_bytes() for f in ("P.txt", "C.txt")}
    assert all(kept.values())
    for f in kept:
        (d / f).unlink()
    both = cli(["-i", "full.gz", "-a", "once.fa", *others, "-E", "E_both.txt", "-I", "3", "-w", "10", "-o", "o.txt", "-t", "1"], d)
    for f, text in kept.items():
        assert (d / f).read_bytes() == text, f
    for head in (b"profile: ", b"cover: "):
        assert line_of(both.stdout, head) == line_of(alone.stdout, head) and len(line_of(alone.stdout, head)) == 1
    assert line_of(alone.stdout, b"abundance: ") == []
    text, line = wanted(lists, s.G, 10, 3)
    assert (d / "E_both.txt").read_bytes() == text
    assert line_of(both.stdout, b"abundance: ") == [line]
    assert both.stdout.index(b"abundance: ") > both.stdout.index(b"cover: ") > both.stdout.index(b"profile: ")


def test_pairs(work):
    """-2: a read pair is one query; the yardstick's rows of the pairs (tests/pairs_ref.py) under the same rule"""
    s, d, _ = work
    pairs = [(r[:len(r) // 2], r[len(r) // 2:]) for r in s.reads[:PAIRS]]
    (d / "m1.fa").write_bytes(records([p[0] for p in pairs]))
    (d / "m2.fa").write_bytes(records([p[1] for p in pairs]))
    rows, _ = pr.rows(s.o, pairs)
    lists = cr.per_query(s.o, rows, 10, 0.5 * s.par[4])
    text, line = wanted(lists, s.G, 10, 5)
    assert sr.pool_of(lists, 10, s.G).lists and sr.pool_of(lists, 10, s.G).settled
    r = cli(["-i", "full.gz", "-a", "m1.fa", "-2", "m2.fa", "-E", "E_pairs.txt", "-I", "5", "-w", "10", "-o", "o.txt", "-t", "1"], d)
    assert (d / "E_pairs.txt").read_bytes() == text
    assert line_of(r.stdout, b"abundance: ") == [line]


def test_refusals_that_need_the_device_list(work):
    """several GPUs in the process, one process per GPU: -P's refusals, for -E"""
    _, d, _ = work
    for devices, env in (("0,0", None), ("0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"})):
        r = cli(["-i", "full.gz", "-a", "once.fa", "-E", "no.txt", "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
        assert r.returncode == 1 and b"-E is not supported" in r.stdout and b"Using " not in r.stdout
        assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_file_that_cannot_be_written(work):
    _, d, _ = work
    r = cli(["-i", "full.gz", "-a", "once.fa", "-E", "no_such_dir/E.txt", "-w", "10", "-o", "o_w.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-E: cannot write no_such_dir/E.txt" in r.stdout
