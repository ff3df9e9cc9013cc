"""`miekki -a <mates 1> -2 <mates 2>`: read pairs as one query each, through the plain output, -n and the profile flags over
query_file's super-batches.  The yardstick is tests/pairs_ref.py (the oracle's sketches of the mates, merged and gated) under
the formatters of the other command-line tests: the files' bytes and the summary lines are what its rows format to."""
import gzip

import numpy as np
import pytest

import clade_ref as cr
import cover_ref as cv
import depth_ref as dr
import gather_ref as gr
import lca_ref as lr
import pairs_ref as pr
import synth
import tally_ref as tr
import winners_ref as wr
from cli_util import cli, line_of

pytestmark = pytest.mark.gpu
REPEATS = 56                       # 56 x 301 pairs: more than one super-batch of 16,384
NODES = lr.preorder([(0, 300), (0, 100), (10, 20), (12, 13), (100, 250), (120, 121), (260, 280)])


def records(reads, tag):
    return b"".join(b">%s%d\n%s\n" % (tag, i, r) for i, r in enumerate(reads))


def said_of(out):
    """what the run said under -2, from the flag on (progress marks may stand before it)"""
    return [l[l.index(b"-2: "):] for l in out.split(b"\n") if b"-2: " in l]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """the 8-bit sample as a dumped index; its 300 pairs as r1.fa / r2.fa with a pair whose mates are both shorter than k (not
    run) and a pair whose mate 2 alone is (run: the read mate 1), 56 times over; the yardstick's rows of the 301 pairs run"""
    s = pr.Sample(8)
    d = tmp_path_factory.mktemp("pairs")
    for g, seq in enumerate(s.seqs):
        (d / f"g{g}.fa").write_bytes(synth.fasta(f"g{g}", seq))
    (d / "genomes.lst").write_bytes(b"".join(b"g%d.fa\n" % g for g in range(len(s.seqs))))
    k, h, fp_bits, b, threshold = s.par
    base = ["-k", str(k), "-h", str(h), "-f", str(fp_bits - 5), "-b", str(b), "-s", str(threshold), "-t", "1"]
    a0, b0 = s.pairs[0]
    both_short = (a0[:k - 1], b0[:k - 2])
    one_short = (s.pairs[1][0], b0[:k - 1])
    given = [both_short] + s.pairs[:150] + [one_short] + s.pairs[150:]
    run = [p for p in given if p != both_short]
    heads = [b">m%d" % i for i, p in enumerate(given) if p != both_short]
    (d / "r1.fa").write_bytes(records([p[0] for p in given], b"m") * REPEATS)
    (d / "r2.fa").write_bytes(records([p[1] for p in given], b"other") * REPEATS)
    (d / "r2.fa.gz").write_bytes(gzip.compress(records([p[1] for p in given], b"other") * REPEATS, 1))
    (d / "once1.fa").write_bytes(records([p[0] for p in given], b"m"))
    (d / "once2.fa").write_bytes(records([p[1] for p in given], b"other"))
    cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
    rows, _ = pr.rows(s.o, run, s.stored)
    assert len(run) == 301 and REPEATS * len(run) > 16384
    assert np.array_equal(rows[150], s.o.query_sequences([one_short[0]])[0])
    return s, d, run, heads, rows


def lines(o, heads, rows, n, thr):
    return b"".join(o.format_query_line(hd, o.filter_results(row, n, 10, 0.5 * thr)) for hd, row in zip(heads, rows))


def test_plain_output_is_one_line_per_pair_under_mate_ones_head(work):
    s, d, run, heads, rows = work
    thr = s.par[4]
    cli(["-i", "full.gz", "-a", "r1.fa", "-2", "r2.fa", "-o", "out.txt", "-t", "1"], d)
    once = lines(s.o, heads, rows, 10, thr)
    assert once.count(b"\n") == 301 and once.count(b";") > 200
    assert (d / "out.txt").read_bytes() == once * REPEATS
    # the gzip'd mate file
    cli(["-i", "full.gz", "-a", "r1.fa", "-2", "r2.fa.gz", "-o", "out_gz.txt", "-t", "1"], d)
    assert (d / "out_gz.txt").read_bytes() == once * REPEATS


def test_every_genome_above_the_thresholds(work):
    s, d, run, heads, rows = work
    cli(["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-n", "0", "-o", "out_n0.txt", "-t", "1"], d)
    assert (d / "out_n0.txt").read_bytes() == lines(s.o, heads, rows, s.o.index_size, s.par[4])
    cli(["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-n", "1", "-o", "out_n1.txt", "-t", "1"], d)
    assert (d / "out_n1.txt").read_bytes() == lines(s.o, heads, rows, 1, s.par[4])


@pytest.mark.parametrize("mate_file", ["r2.fa", "r2.fa.gz"])
def test_the_profiles_in_one_run(work, mate_file):
    s, d, run, heads, rows = work
    o, thr = s.o, s.par[4]
    k, h, fp_bits = s.par[:3]
    n = REPEATS * len(run)
    tree, names = lr.Tree(NODES, o.index_size), lr.names_of(NODES)
    (d / "tax.txt").write_bytes(lr.taxonomy_file(NODES, names))
    tally = tr.tally(o, rows, 10, 0.5 * thr) * np.uint64(REPEATS)
    seen = pr.seen(o, run)
    cov = cv.covered(o, seen, s.stored)
    t, per_read = lr.lca_tally(cr.per_query(o, rows, 10, 0.5 * thr), tree, 10)
    t = t * np.uint64(REPEATS)
    assert tally[:, 2].sum() > 200 * REPEATS and (cov > 0).sum() > 100 and len({int(v) for v in per_read}) > 3
    r = cli(["-i", "full.gz", "-a", "r1.fa", "-2", mate_file, "-P", "P.txt", "-C", "C.txt", "-T", "tax.txt", "-y", "y.txt", "-Y", "Y.txt",
             "-m", "10", "-o", "o.txt", "-t", "1"], d)
    assert (d / "P.txt").read_bytes() == tr.format_profile(tally)
    assert (d / "C.txt").read_bytes() == cv.format_cover(cov, o.sketch_size)
    assert (d / "y.txt").read_bytes() == lr.format_report(t, tree, names)
    assert (d / "Y.txt").read_bytes() == lr.format_reads(np.tile(per_read, REPEATS))
    assert line_of(r.stdout, b"profile: ") == [tr.summary_line(tally, n)]
    assert line_of(r.stdout, b"cover: ") == [cv.summary_line(n, seen.sum(), h, fp_bits, cov)]
    assert line_of(r.stdout, b"lca: ") == [lr.summary_line(t, n, 10)]
    assert (d / "o.txt").read_bytes() == b""
    for f in ("P.txt", "C.txt", "y.txt", "Y.txt"):
        (d / f).unlink()


def test_the_other_sinks_take_pairs_too(work):
    """-L -p, -W, -D, -G -g in one run over the pairs once: the yardsticks of their own tests over the pairs' rows and cells"""
    s, d, run, heads, rows = work
    o, thr = s.o, s.par[4]
    k, h, fp_bits = s.par[:3]
    n, ss = len(run), o.sketch_size
    lists = cr.per_query(o, rows, 10, 0.5 * thr)
    text, clade = cr.clade_file(cr.from_cuts((0, 100, 250, 300)))
    (d / "clades.txt").write_bytes(text)
    ct = cr.clade_tally(lists, clade)
    seen = pr.seen(o, run)
    cov = cv.covered(o, seen, s.stored)
    w, claimed = wr.won(o, seen, s.stored, wr.order(cov, ss))
    m = np.zeros((o.P, 1 << fp_bits), np.int64)
    for fp in pr.sketches(o, run):
        live = np.flatnonzero(fp != cv.empty_of(o))
        m[live, fp[live].astype(np.int64)] += 1
    assert np.array_equal(m > 0, seen) and m.max() < 255
    tab = dr.table(m)
    med, total, dcov = dr.profile(o, tab, s.stored)
    assert np.array_equal(dcov, cov)
    picks, cells, explained = gr.gather(o, seen, s.stored, min_new=10, table=tab)
    assert len(picks) > 20
    r = cli(["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-L", "clades.txt", "-p", "p.txt", "-W", "W.txt", "-D", "D.txt",
             "-G", "G.txt", "-g", "10", "-o", "o_sinks.txt", "-t", "1"], d)
    assert (d / "p.txt").read_bytes() == cr.format_clade_profile(ct, clade)
    assert (d / "W.txt").read_bytes() == wr.format_winners(w, cov, ss)
    assert (d / "D.txt").read_bytes() == dr.format_depth(med, total, dcov, ss)
    assert (d / "G.txt").read_bytes() == gr.format_gather(picks, with_depth=True)
    assert line_of(r.stdout, b"clades: ") == [cr.summary_line(ct, n)]
    assert line_of(r.stdout, b"winners: ") == [wr.summary_line(n, claimed, seen.sum(), w)]
    assert line_of(r.stdout, b"depth: ") == [dr.summary_line(n, seen.sum(), 0, h, fp_bits, dcov)]
    assert line_of(r.stdout, b"gather: ") == [gr.summary_line(n, explained, cells, len(picks), 10)]


@pytest.mark.parametrize("args,devices,env", [
    (["-i", "full.gz", "-2", "once2.fa"], "0", None),                                                       # without -a
    (["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-e"], "0", None),
    (["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-A", "genomes.lst"], "0", None),
    (["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-X"], "0", None),
    (["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-S", "genomes.lst", "-c", "no.txt"], "0", None),
    (["-i", "full.gz", "-a", "once1.fa", "-2", "no_such_mates.fa"], "0", None),
    (["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa", "-P", "no.txt"], "0,0", None),                  # several GPUs in the process
    (["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa"], "0,0", None),
    (["-i", "full.gz", "-a", "once1.fa", "-2", "once2.fa"], "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}),
])
def test_refusals_name_the_flag_and_leave_no_file(work, args, devices, env):
    _, d, _, _, _ = work
    r = cli([*args, "-o", "no_out.txt"], d, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and b"-2" in r.stdout, r.stdout
    assert b"Using " not in r.stdout                                       # before any device is touched
    assert not (d / "no.txt").exists() and not (d / "no_out.txt").exists()


def test_a_mate_file_one_record_short(work):
    s, d, run, heads, rows = work
    whole = (d / "once2.fa").read_bytes()
    short = whole[:whole.rstrip(b"\n").rfind(b">")]
    assert short.count(b">") == 301
    (d / "short2.fa").write_bytes(short)
    for a, m, name in (("once1.fa", "short2.fa", b"short2.fa"), ("short2.fa", "once1.fa", b"short2.fa")):
        r = cli(["-i", "full.gz", "-a", a, "-2", m, "-P", "P_short.txt", "-C", "C_short.txt", "-o", "o_short.txt", "-t", "1"], d, ok=False)
        assert r.returncode == 1, r.stdout
        said = said_of(r.stdout)
        assert len(said) == 1 and said[0].startswith(b"-2: " + name + b" ends after 301 records"), r.stdout
        assert not (d / "P_short.txt").exists() and not (d / "C_short.txt").exists()


def test_a_pair_beyond_the_short_sketch(work):
    s, d, run, heads, rows = work
    k = s.par[0]
    text = b"".join(s.seqs[:4])
    a, b = s.pairs[0]
    (d / "long1.fa").write_bytes(records([a[:k - 1], a, a, text[:2100]], b"x"))
    (d / "long2.fa").write_bytes(records([b[:k - 1], b, b, text[3000:5100]], b"y"))
    r = cli(["-i", "full.gz", "-a", "long1.fa", "-2", "long2.fa", "-P", "P_long.txt", "-o", "o_long.txt", "-t", "1"], d, ok=False)
    assert r.returncode == 1, r.stdout
    said = said_of(r.stdout)
    # the pair's ordinal counts the pairs that are run, as -Y's does: the first record is not
    assert len(said) == 1 and said[0].startswith(b"-2: pair 2 (>x3) holds %d k-mers" % (2 * (2100 - k))), r.stdout
    assert not (d / "P_long.txt").exists()
    # one k-mer fewer each: 4,096 in all, taken
    (d / "fits1.fa").write_bytes(records([text[:2048 + k]], b"x"))
    (d / "fits2.fa").write_bytes(records([text[3000:3000 + 2048 + k]], b"y"))
    cli(["-i", "full.gz", "-a", "fits1.fa", "-2", "fits2.fa", "-o", "o_fits.txt", "-t", "1"], d)
    want, _ = pr.rows(s.o, [(text[:2048 + k], text[3000:3000 + 2048 + k])], s.stored)
    assert (d / "o_fits.txt").read_bytes() == lines(s.o, [b">x0"], want, 10, s.par[4])
