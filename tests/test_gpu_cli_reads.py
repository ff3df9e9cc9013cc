"""FASTQ read files and `miekki -q <int>`: four-line records wherever reads are read (-a, -2, -S), run as their sequences without
-q and cut at their bad bases with it.  The yardstick is tests/reads_ref.py (the oracle's sketches of the segments, merged and
gated) under the formatters of the other command-line tests: the files' bytes and the summary lines are what its rows format
to."""
import gzip

import numpy as np
import pytest

import cover_ref as cv
import pairs_ref as pr
import panel_ref as pn
import reads_ref as rr
import synth
import tally_ref as tr
from cli_util import cli, line_of

pytestmark = pytest.mark.gpu
Q = rr.MIN_QUAL


def fastq(reads, tag):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, x) for i, (s, x) in enumerate(reads))


def twin(reads, tag):
    """the 2-line file with the same head lines"""
    return b"".join(b"@%s%d\n%s\n" % (tag, i, s) for i, (s, _) in enumerate(reads))


def lines(o, heads, rows, n, thr):
    return b"".join(o.format_query_line(hd, o.filter_results(row, n, 10, 0.5 * thr)) for hd, row in zip(heads, rows))


def quality_line(k, q, queries):
    bad, bases, none = rr.quality_counts(k, q, queries)
    return b"quality: %d of %d bases below %d, %d of %d queries without a k-mer left" % (bad, bases, q, none, len(queries))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the 8-bit sample as a dumped index; 200 pairs with qualities as m1.fq / m2.fq with a pair whose mates are both shorter
    than k (never run), one whose mate 1 alone is, and a read that is all bad; the 2-line twins of both files"""
    s = pr.Sample(8)
    d = tmp_path_factory.mktemp("reads")
    for g, seq in enumerate(s.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(len(s.seqs))))
    k, h, fp_bits, b, threshold = s.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    sample = rr.sample_reads(s.seqs)
    (a0, x0), (b0, y0) = sample[0]
    given = ([((a0[:k - 1], x0[:k - 1]), (b0[:k - 2], y0[:k - 2]))] + sample[:90] + [((a0[:k - 1], x0[:k - 1]), sample[1][1])] +
             [((a0, rr.mask(len(a0), range(len(a0)))), (b0, rr.mask(len(b0), range(0, len(b0), k))))] + sample[90:])
    m1, m2 = [p[0] for p in given], [p[1] for p in given]
    for name, data in (("m1.fq", fastq(m1, b"m")), ("m2.fq", fastq(m2, b"other")), ("m1.fa", twin(m1, b"m")), ("m2.fa", twin(m2, b"other"))):
        (d / name).write_bytes(data)
        (d / (name + ".gz")).write_bytes(gzip.compress(data, 1))
    return s, d, given


def kept_singles(given, k):
    """(heads, queries) of the records of m1.fq that are run"""
    keep = [(i, p[0]) for i, p in enumerate(given) if len(p[0][0]) >= k]
    return [b"@m%d" % i for i, _ in keep], [(r,) for _, r in keep]


def kept_pairs(given, k):
    keep = [(i, p) for i, p in enumerate(given) if len(p[0][0]) >= k or len(p[1][0]) >= k]
    return [b"@m%d" % i for i, _ in keep], [p for _, p in keep]


@pytest.mark.parametrize("ext", ["", ".gz"])
def test_a_fastq_file_is_its_two_line_twin_without_q(work, ext):
    s, d, given = work
    o, thr, k = s.o, s.par[4], s.par[0]
    heads, queries = kept_singles(given, k)
    want = lines(o, heads, o.query_sequences([q[0][0] for q in queries]), 10, thr)
    assert want.count(b"\n") == 201 and want.count(b";") > 20
    outs = {}
    for kind in ("fq", "fa"):
        r = cli(["-i", "full.gz", "-a", "m1.%s%s" % (kind, ext), "-o", "plain_%s.txt" % kind, "-t", "1"], d)
        assert not line_of(r.stdout, b"quality: ")
        cli(["-i", "full.gz", "-a", "m1.%s%s" % (kind, ext), "-P", "P_%s.txt" % kind, "-C", "C_%s.txt" % kind, "-o", "o_%s.txt" % kind, "-t", "1"], d)
        outs[kind] = [(d / (f % kind)).read_bytes() for f in ("plain_%s.txt", "P_%s.txt", "C_%s.txt")]
    assert outs["fq"] == outs["fa"]
    assert outs["fq"][0] == want and len(outs["fq"][1]) > 100 and len(outs["fq"][2]) > 100


@pytest.mark.parametrize("ext", ["", ".gz"])
def test_pairs_of_fastq_files_are_the_pairs_of_their_twins_without_q(work, ext):
    s, d, given = work
    o, thr, k = s.o, s.par[4], s.par[0]
    cli(["-i", "full.gz", "-a", "m1.fq" + ext, "-2", "m2.fq" + ext, "-o", "pairs_fq.txt", "-t", "1"], d)
    cli(["-i", "full.gz", "-a", "m1.fa" + ext, "-2", "m2.fa" + ext, "-o", "pairs_fa.txt", "-t", "1"], d)
    pheads, pq = kept_pairs(given, k)
    assert (d / "pairs_fq.txt").read_bytes() == (d / "pairs_fa.txt").read_bytes() == lines(o, pheads, rr.rows(o, 0, pq, s.stored)[0], 10, thr)


def test_q_cuts_the_reads_of_a(work):
    s, d, given = work
    o, thr = s.o, s.par[4]
    k, h, fp_bits = s.par[:3]
    heads, queries = kept_singles(given, k)
    rows, active = rr.rows(o, Q, queries, s.stored)
    assert not np.array_equal(rows, o.query_sequences([q[0][0] for q in queries]))
    n = len(queries)
    r = cli(["-i", "full.gz", "-a", "m1.fq", "-q", str(Q), "-o", "q_plain.txt", "-t", "1"], d)
    assert (d / "q_plain.txt").read_bytes() == lines(o, heads, rows, 10, thr)
    assert line_of(r.stdout, b"quality: ") == [quality_line(k, Q, queries)]
    cli(["-i", "full.gz", "-a", "m1.fq.gz", "-q", str(Q), "-n", "0", "-o", "q_n0.txt", "-t", "1"], d)
    assert (d / "q_n0.txt").read_bytes() == lines(o, heads, rows, o.index_size, thr)
    tally = tr.tally(o, rows, 10, 0.5 * thr)
    seen = rr.seen(o, Q, queries)
    cov = cv.covered(o, seen, s.stored)
    r = cli(["-i", "full.gz", "-a", "m1.fq", "-q", str(Q), "-P", "qP.txt", "-C", "qC.txt", "-o", "qo.txt", "-t", "1"], d)
    assert (d / "qP.txt").read_bytes() == tr.format_profile(tally)
    assert (d / "qC.txt").read_bytes() == cv.format_cover(cov, o.sketch_size)
    assert line_of(r.stdout, b"profile: ") == [tr.summary_line(tally, n)]
    assert line_of(r.stdout, b"cover: ") == [cv.summary_line(n, seen.sum(), h, fp_bits, cov)]
    assert line_of(r.stdout, b"quality: ") == [quality_line(k, Q, queries)]
    # -q 0 is the run without -q, plus its line
    r = cli(["-i", "full.gz", "-a", "m1.fq", "-q", "0", "-o", "q0.txt", "-t", "1"], d)
    assert (d / "q0.txt").read_bytes() == lines(o, heads, o.query_sequences([q[0][0] for q in queries]), 10, thr)
    assert line_of(r.stdout, b"quality: ") == [quality_line(k, 0, queries)]


def test_q_cuts_the_pairs_of_2(work):
    s, d, given = work
    o, thr = s.o, s.par[4]
    k, h, fp_bits = s.par[:3]
    heads, queries = kept_pairs(given, k)
    rows, _ = rr.rows(o, Q, queries, s.stored)
    n = len(queries)
    assert n == 202
    tally = tr.tally(o, rows, 10, 0.5 * thr)
    seen = rr.seen(o, Q, queries)
    cov = cv.covered(o, seen, s.stored)
    r = cli(["-i", "full.gz", "-a", "m1.fq", "-2", "m2.fq.gz", "-q", str(Q), "-o", "q2.txt", "-t", "1"], d)
    assert (d / "q2.txt").read_bytes() == lines(o, heads, rows, 10, thr)
    assert line_of(r.stdout, b"quality: ") == [quality_line(k, Q, queries)]
    r = cli(["-i", "full.gz", "-a", "m1.fq", "-2", "m2.fq", "-q", str(Q), "-P", "q2P.txt", "-C", "q2C.txt", "-o", "q2o.txt", "-t", "1"], d)
    assert (d / "q2P.txt").read_bytes() == tr.format_profile(tally)
    assert (d / "q2C.txt").read_bytes() == cv.format_cover(cov, o.sketch_size)
    assert line_of(r.stdout, b"profile: ") == [tr.summary_line(tally, n)]
    assert line_of(r.stdout, b"cover: ") == [cv.summary_line(n, seen.sum(), h, fp_bits, cov)]


def test_the_samples_of_S_may_be_fastq(work):
    s, d, given = work
    o = s.o
    k, h, fp_bits = s.par[:3]
    (d / "fq.lst").write_bytes(b"m1.fq\nm2.fq.gz\n")
    (d / "fa.lst").write_bytes(b"m1.fa\nm2.fa.gz\n")
    samples = [[(p[0],) for p in given if len(p[0][0]) >= k], [(p[1],) for p in given if len(p[1][0]) >= k]]
    for q, lst, out in ((None, "fq.lst", "S_fq.txt"), (None, "fa.lst", "S_fa.txt"), (Q, "fq.lst", "S_q.txt")):
        r = cli(["-i", "full.gz", "-S", lst, "-c", out, "-o", "So.txt", "-t", "1", *(["-q", str(q)] if q is not None else [])], d)
        seens = [rr.seen(o, q or 0, sample) for sample in samples]
        cov = pn.covered(o, seens, s.stored)
        assert (d / out).read_bytes() == pn.format_panel(cov, o.sketch_size), (q, lst)
        for i in range(2):
            assert line_of(r.stdout, b"panel[%d]: " % i) == [pn.sample_line(i, len(samples[i]), int(seens[i].sum()), h, fp_bits, cov[i])]
        assert line_of(r.stdout, b"quality: ") == ([] if q is None else [quality_line(k, q, samples[0] + samples[1])])
    assert (d / "S_fq.txt").read_bytes() == (d / "S_fa.txt").read_bytes() != (d / "S_q.txt").read_bytes()


@pytest.mark.parametrize("args,devices,env,names", [
    (["-i", "full.gz", "-q", "20"], "0", None, b"-a or -S"),
    (["-i", "full.gz", "-a", "m1.fq", "-q", "20", "-e"], "0", None, b"-e"),
    (["-i", "full.gz", "-a", "m1.fq", "-q", "20", "-A", "genomes.lst"], "0", None, b"-A"),
    (["-i", "full.gz", "-q", "20", "-X"], "0", None, b"-q"),
    (["-i", "full.gz", "-a", "m1.fq", "-q", "94"], "0", None, b"0 .. 93"),
    (["-i", "full.gz", "-a", "m1.fq", "-q", "-1"], "0", None, b"0 .. 93"),
    (["-i", "full.gz", "-a", "m1.fq", "-q", "2x"], "0", None, b"0 .. 93"),
    (["-i", "full.gz", "-a", "m1.fa", "-q", "20"], "0", None, b"m1.fa is not a FASTQ file"),
    (["-i", "full.gz", "-a", "m1.fa.gz", "-q", "20", "-P", "no.txt"], "0", None, b"m1.fa.gz is not a FASTQ file"),
    (["-i", "full.gz", "-a", "m1.fq", "-2", "m2.fa", "-q", "20"], "0", None, b"m2.fa is not a FASTQ file"),
    (["-i", "full.gz", "-S", "mixed.lst", "-c", "no.txt", "-q", "20"], "0", None, b"m2.fa.gz is not a FASTQ file"),
    (["-i", "full.gz", "-a", "m1.fq", "-q", "20"], "0,0", None, b"several GPUs"),
    (["-i", "full.gz", "-a", "m1.fq", "-q", "20", "-P", "no.txt"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}, b"one process per GPU"),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env, names):
    _, d, _ = work
    (d / "mixed.lst").write_bytes(b"m1.fq\nm2.fa.gz\n")
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and b"-q" in r.stdout and names in r.stdout, r.stdout
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_mid_run_errors_name_the_file_and_the_record(work):
    s, d, given = work
    k = s.par[0]
    whole = (d / "m1.fq").read_bytes()
    cut = whole[:whole.rstrip(b"\n").rfind(b"\n")]                          # the last record without its quality line
    bad_qual = whole.replace(b"\n+\n", b"\n+\nI", 1)                        # record 0: one quality too many
    (d / "cut.fq").write_bytes(cut)
    (d / "bad_qual.fq").write_bytes(bad_qual)
    for name, word in (("cut.fq", b"cut.fq: FASTQ record %d is cut short" % (len(given) - 1)), ("bad_qual.fq", b"bad_qual.fq: FASTQ record 0 has ")):
        for extra in ([], ["-q", "20"]):
            r = cli(["-i", "full.gz", "-a", name, "-P", "P_bad.txt", "-C", "C_bad.txt", "-o", "o_bad.txt", "-t", "1", *extra], d, ok=False)
            assert r.returncode == 1 and word in r.stdout, r.stdout
            assert not (d / "P_bad.txt").exists() and not (d / "C_bad.txt").exists()
    r = cli(["-i", "full.gz", "-a", "m1.fq", "-2", "cut.fq", "-P", "P_bad.txt", "-o", "o_bad.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"cut.fq: FASTQ record %d is cut short" % (len(given) - 1) in r.stdout and not (d / "P_bad.txt").exists()


def test_q_ends_the_run_at_a_read_or_pair_of_more_than_4096_bases(work):
    """the ordinal counts the records that are run"""
    s, d, given = work
    k = s.par[0]
    text = b"".join(s.seqs[:3])
    long1 = [(text[:k - 1], rr.mask(k - 1)), (text[:100], rr.mask(100)), (text[:4097], rr.mask(4097))]
    long2 = [(text[:k - 1], rr.mask(k - 1)), (text[:100], rr.mask(100)), (text[:97], rr.mask(97))]
    (d / "long1.fq").write_bytes(fastq(long1, b"x"))
    (d / "long2.fq").write_bytes(fastq(long2, b"y"))
    r = cli(["-i", "full.gz", "-a", "long1.fq", "-q", "20", "-P", "P_long.txt", "-o", "o_long.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-q: read 1 (@x2) of long1.fq holds 4097 bases" in r.stdout and not (d / "P_long.txt").exists()
    long1[2] = (text[:4000], rr.mask(4000))
    (d / "long1.fq").write_bytes(fastq(long1, b"x"))
    r = cli(["-i", "full.gz", "-a", "long1.fq", "-2", "long2.fq", "-q", "20", "-P", "P_long.txt", "-o", "o_long.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1 and b"-q: pair 1 (@x2) holds 4097 bases" in r.stdout and not (d / "P_long.txt").exists()
    # without -q the long read is a long read
    cli(["-i", "full.gz", "-a", "long1.fq", "-o", "o_long_plain.txt", "-t", "1"], d)
    assert (d / "o_long_plain.txt").read_bytes().count(b"\n") == 2
