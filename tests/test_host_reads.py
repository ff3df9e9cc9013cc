"""host/reads.hpp without a GPU, through tests/helpers/reads_check.cpp built with -fsanitize=address,undefined: 2-line files come
out as the reader before FASTQ read them, FASTQ files plain and gzip'd give their records, records may straddle the 4 MiB read
buffer, every format error names the file and the record, and the `quality:` line counts what tests/reads_ref.py counts."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import reads_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 31


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("reads_check")
    exe = str(d / "reads_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-o", exe, os.path.join(ROOT, "tests", "helpers", "reads_check.cpp"), "-lz"],
                   check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], cwd=d, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
        return r.stdout
    return d, run


def records(n, seed, lo=20, hi=300):
    """[(head, seq, qual)] with heads that carry blanks and '+', sequences with N and lower case, every printable quality"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(rng.integers(lo, hi))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTNacgt", np.uint8), L))
        qual = bytes(rng.integers(33, 127, L, dtype=np.uint8))
        out.append((b"@read%d len=%d +x" % (i, L), seq, qual))
    return out


def fastq(recs, plus=b"+"):
    return b"".join(h + b"\n" + s + b"\n" + plus + b"\n" + q + b"\n" for h, s, q in recs)


def lines(recs, k=0):
    return b"".join(h + b"\t" + s + b"\t" + q + b"\n" for h, s, q in recs if len(s) >= k)


def write(d, name, data):
    p = str(d / name)
    with (gzip.open(p, "wb", compresslevel=1) if name.endswith(".gz") else open(p, "wb")) as f:
        f.write(data)
    return p


def test_two_line_files_are_read_as_before(tool):
    d, run = tool
    recs = records(500, 1)
    texts = {
        "plain.fa": b"".join(b">" + h[1:] + b"\n" + s + b"\n" for h, s, _ in recs),
        "no_newline.fa": b">a\nACGT" * 1 + b"\n>b\n" + b"ACGTTGCA" * 8,
        "odd_lines.fa": b">a\n" + b"ACGT" * 10 + b"\n>b",
        "blank_lines.fa": b">a\n\n" + b"ACGT" * 10 + b"\n>b\n" + b"G" * 40 + b"\n\n\n",
        "quality_head.txt": b"+@\n" + b"ACGT" * 10 + b"\n@later\n" + b"T" * 50 + b"\n",
        "at_heads.fa": b"".join(h + b"\n" + s + b"\n" for h, s, _ in recs),       # 2-line records whose heads start with '@'
        "at_heads_one.fa": b"@only\n" + b"ACGT" * 10 + b"\n",
        "at_head_alone.fa": b"@only\n",
        "at_four_lines.fa": b"@only\nACGT\n-\nIIII\n",                           # no '+' on its third line: two 2-line records
        "crlf.fa": b">a\r\n" + b"ACGT" * 10 + b"\r\n",
        "empty.fa": b"",
        "newline_only.fa": b"\n",
    }
    rng = np.random.default_rng(5)
    big = []
    while sum(map(len, big)) < 9 << 20:                           # more than two read buffers of records of every length
        L = int(rng.integers(0, 5000))
        big.append(b">r%d\n" % len(big) + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)) + b"\n")
    texts["big.fa"] = b"".join(big)
    for name, data in texts.items():
        for path in (write(d, name, data), write(d, name + ".gz", data)):
            assert run("isfastq", path) == b"0\n", name
            for want in (1, 7, 16384):
                if name == "big.fa" and want == 1:
                    continue
                out = run("old", K, want, path)
                assert out.startswith(b"same "), (name, want, out)
            if name == "big.fa":
                assert out == b"same %d\n" % sum(1 for r in big if len(r.split(b"\n")[1]) >= K)
    # and what the records are: pairs of lines, the last one's sequence empty when the file has an odd number
    assert run("records", str(d / "odd_lines.fa")) == b"fastq 0\n>a\t" + b"ACGT" * 10 + b"\t\n>b\t\t\n"
    assert run("records", str(d / "empty.fa")) == b"fastq 0\n"


@pytest.mark.parametrize("gz", [False, True])
def test_fastq_records(tool, gz):
    d, run = tool
    ext = ".fq.gz" if gz else ".fq"
    recs = records(700, 2)
    path = write(d, "reads" + ext, fastq(recs))
    assert run("isfastq", path) == b"1\n"
    assert run("records", path) == b"fastq 1\n" + lines(recs)
    for want in (1, 7, 16384):
        assert run("dump", K, want, path) == b"fastq 1\n" + lines(recs, K)
    # the third line may repeat the head
    path = write(d, "plus_head" + ext, b"".join(h + b"\n" + s + b"\n+" + h[1:] + b"\n" + q + b"\n" for h, s, q in recs[:50]))
    assert run("dump", 0, 9, path) == b"fastq 1\n" + lines(recs[:50])
    # one record without a final newline; an empty file is no FASTQ file and has no record
    one = recs[3]
    path = write(d, "one" + ext, fastq([one])[:-1])
    assert run("records", path) == b"fastq 1\n" + lines([one])
    assert run("dump", 0, 1, write(d, "empty" + ext, b"")) == b"fastq 0\n"
    # a quality line that starts with '@', a sequence of no bases
    odd = [(b"@a", b"ACGT", b"@III"), (b"@b", b"", b""), (b"@c", b"AC", b"+@")]
    assert run("records", write(d, "odd" + ext, fastq(odd))) == b"fastq 1\n" + lines(odd)


def test_fastq_records_straddle_the_read_buffer(tool):
    d, run = tool
    rng = np.random.default_rng(9)
    recs = []
    size = 0
    while size < 9 << 20:                                         # two refills of the 4 MiB buffer, a boundary in every kind of line
        L = int(rng.integers(0, 4000))
        seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L))
        recs.append((b"@r%d" % len(recs), seq, bytes(rng.integers(33, 127, L, dtype=np.uint8))))
        size += 2 * L + len(recs[-1][0]) + 5
    data = fastq(recs)
    at = {(4 << 20) - 1, 4 << 20, 8 << 20}
    assert all(a < len(data) for a in at)
    for path in (write(d, "big.fq", data), write(d, "big.fq.gz", data)):
        assert run("dump", K, 16384, path) == b"fastq 1\n" + lines(recs, K)
    assert run("records", str(d / "big.fq")) == b"fastq 1\n" + lines(recs)


def test_format_errors_name_the_file_and_the_record(tool):
    d, run = tool
    recs = records(40, 3, lo=40)
    good = fastq(recs)
    h, s, q = recs[7]
    cases = {
        "cut_head.fq": (fastq(recs[:9]) + b"@last\n", 9, b"cut short"),
        "cut_seq.fq": (fastq(recs[:9]) + b"@last\nACGT\n", 9, b"cut short"),
        "cut_plus.fq": (fastq(recs[:9]) + b"@last\nACGT\n+\n", 9, b"cut short"),
        "no_plus.fq": (fastq(recs[:7]) + h + b"\n" + s + b"\n" + s + b"\n" + q + b"\n" + fastq(recs[8:]), 7, b"does not start with '+'"),
        "multi_line.fq": (fastq(recs[:7]) + h + b"\n" + s[:20] + b"\n" + s[20:] + b"\n+\n" + q + b"\n", 7, b"does not start with '+'"),
        "short_qual.fq": (fastq(recs[:7]) + h + b"\n" + s + b"\n+\n" + q[:-1] + b"\n" + fastq(recs[8:]), 7, b"%d bases and %d qualities" % (len(s), len(s) - 1)),
        "long_qual.fq": (fastq(recs[:7]) + h + b"\n" + s + b"\n+\n" + q + b"I\n" + fastq(recs[8:]), 7, b"%d bases and %d qualities" % (len(s), len(s) + 1)),
    }
    for name, (data, ordinal, word) in cases.items():
        for path in (write(d, name, data), write(d, name + ".gz", data)):
            out = run("dump", 0, 5, path)
            body, _, err = out.partition(b"error: ")
            assert body == b"fastq 1\n" + lines(recs[:ordinal] if ordinal else []), name
            assert err.startswith(path.encode() + b": FASTQ record %d" % ordinal) and word in err, (name, err)
    assert b"error" not in run("dump", 0, 5, write(d, "good.fq", good))


def test_pairs_of_fastq_files_and_the_limit(tool):
    d, run = tool
    r1, r2 = records(300, 4), records(300, 5)
    p1, p2 = write(d, "m_1.fq", fastq(r1)), write(d, "m_2.fq.gz", fastq(r2))
    want = b"".join(a[0] + b"\t" + a[1] + b"\t" + b[1] + b"\t" + a[2] + b"\t" + b[2] + b"\n"
                    for a, b in zip(r1, r2) if len(a[1]) >= K or len(b[1]) >= K)
    assert run("pairs", K, 11, p1, p2) == want
    # a format error in either file ends the pairs
    bad = write(d, "m_bad.fq", fastq(r2[:5]) + b"@x\nACGT\n+\nIII\n")
    out = run("pairs", 0, 11, p1, bad)
    assert out.count(b"\n") == 6 and b"error: " + bad.encode() + b": FASTQ record 5" in out
    # more bases than a pair with qualities may hold: the pair's ordinal among the kept ones, and mate 1's head
    long1 = [(b"@s", b"A" * 10, b"I" * 10), (b"@p0", b"ACGT" * 20, b"I" * 80), (b"@p1", b"A" * 4000, b"I" * 4000)]
    long2 = [(b"@s", b"A" * 10, b"I" * 10), (b"@p0", b"ACGT" * 20, b"I" * 80), (b"@p1", b"C" * 97, b"I" * 97)]
    out = run("pairs", K, 11, write(d, "l_1.fq", fastq(long1)), write(d, "l_2.fq", fastq(long2)), 4096)
    assert out.count(b"\n") == 2 and b"error: -q: pair 1 (@p1) holds 4097 bases" in out
    long2[2] = (b"@p1", b"C" * 96, b"I" * 96)
    assert b"error" not in run("pairs", K, 11, str(d / "l_1.fq"), write(d, "l_2.fq", fastq(long2)), 4096)
    out = run("quality", K, 20, write(d, "l_3.fq", fastq(long1[:2] + [(b"@big", b"A" * 4097, b"I" * 4097)])))
    assert b"error: -q: read 1 (@big) of " in out and b"holds 4097 bases" in out


def test_the_quality_line(tool):
    d, run = tool
    for seed, q in ((6, 20), (7, 0), (8, 93), (6, 40)):
        r1, r2 = records(400, seed, lo=10, hi=200), records(400, seed + 10, lo=10, hi=200)
        p1, p2 = write(d, "q_1.fq", fastq(r1)), write(d, "q_2.fq", fastq(r2))
        kept = [((s, x),) for _, s, x in r1 if len(s) >= K]
        assert run("quality", K, q, p1) == ("quality: %d of %d bases below %d, %d of %d queries without a k-mer left\n"
                                           % (*rr.quality_counts(K, q, kept)[:2], q, rr.quality_counts(K, q, kept)[2], len(kept))).encode()
        kept = [((a[1], a[2]), (b[1], b[2])) for a, b in zip(r1, r2) if len(a[1]) >= K or len(b[1]) >= K]
        bad, bases, none = rr.quality_counts(K, q, kept)
        assert run("quality", K, q, p1, p2) == ("quality: %d of %d bases below %d, %d of %d queries without a k-mer left\n" % (bad, bases, q, none, len(kept))).encode()
    # by hand: k = 3, a stretch of four good bases is a k-mer
    p = write(d, "hand.fq", fastq([(b"@a", b"ACGTACGT", b"IIII#III"), (b"@b", b"ACGTACGT", b"III#III#"), (b"@c", b"ACGT", b"####")]))
    assert run("quality", 3, 20, p) == b"quality: 7 of 20 bases below 20, 2 of 3 queries without a k-mer left\n"
