"""`miekki -i a.gz -M b.gz [-M c.gz ...]`: the genomes of further index files behind those of -i, once the index is loaded
and before -K, -F, -R / -r, -d and every query.  The yardstick is never the join: it is the files the existing `-l ... -d`
path wrote -- a list cut in two (in three) and built part by part must join to the file of the whole list -- and, for a file the
reference itself wrote, tests/extend_ref.py: joined_stream, which tests/test_extend_definition.py holds against the oracle."""
import gzip
import os

import numpy as np
import pytest

import extend_ref
import synth
from cli_util import cli

pytestmark = pytest.mark.gpu


def inflate(path, also=()):
    raw = bytearray(gzip.open(path, "rb").read())
    for i in (32, *also):
        raw[i] = 0
    return bytes(raw)


def genomes_of(path):
    """index_size of an index file's header"""
    with gzip.open(path, "rb") as f:
        return extend_ref.HDR.unpack(f.read(39))[4]


class Work:
    """a case's files in a directory of their own, and its genome list whole ("full"), cut in two ("a", "b") and the first of
    those cut again ("p0", "p1"): <key>.gz is what the existing `-l <key>.lst -d <key>.gz` writes, made when first asked for"""

    def __init__(self, name, d):
        self.case, self.d = synth.CASES[name](), d
        case = self.case
        for fn, data, gz in dict((f[0], f) for f in case.genome_files).values():
            (d / fn).write_bytes(gzip.compress(data, 1) if gz else data)
        names = [fn for fn, _, _ in case.genome_files]
        n = len(names)
        assert n >= 5
        self.lists = {"full": names + ["missing_file.fa", "ab"], "a": names[:n // 2 + 1], "b": names[n // 2 + 1:],
                      "p0": names[:1], "p1": names[1:n // 2 + 1]}
        self.base = ["-k", str(case.k), "-h", str(case.h), "-f", str(case.f), "-b", str(case.b), "-s", str(case.threshold), "-t", "1"]
        self.sizes = {}

    def need(self, *keys):
        for key in keys:
            if key not in self.sizes:
                (self.d / f"{key}.lst").write_text("".join(fn + "\n" for fn in self.lists[key]))
                cli(["-l", f"{key}.lst", "-d", f"{key}.gz", "-o", f"build_{key}.txt", *self.base], self.d)
                self.sizes[key] = genomes_of(self.d / f"{key}.gz")
                assert self.sizes[key] > 0, key
        return self


@pytest.fixture(scope="module")
def workdirs(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Work(name, tmp_path_factory.mktemp(name))
        return made[name]
    return get


@pytest.mark.parametrize("name", ["messy", "w16"])
def test_a_build_split_in_two_joins_to_the_whole_build(workdirs, name):
    w = workdirs(name).need("full", "a", "b")
    d, sizes = w.d, w.sizes
    assert sizes["a"] + sizes["b"] == sizes["full"]
    so = cli(["-i", "a.gz", "-M", "b.gz", "-d", "ab.gz", "-o", "o1.txt", "-t", "1"], d).stdout
    assert inflate(d / "ab.gz") == inflate(d / "full.gz")
    assert b"Genomes joined: %d from b.gz, the index holds %d\n" % (sizes["b"], sizes["full"]) in so


@pytest.mark.parametrize("name", ["messy", "w16"])
def test_a_build_split_in_three_joins_to_the_whole_build(workdirs, name):
    w = workdirs(name).need("full", "p0", "p1", "b")
    d, sizes = w.d, w.sizes
    assert sizes["p0"] + sizes["p1"] + sizes["b"] == sizes["full"]
    so = cli(["-i", "p0.gz", "-M", "p1.gz", "-M", "b.gz", "-d", "p01b.gz", "-o", "o2.txt", "-t", "1"], d).stdout
    assert inflate(d / "p01b.gz") == inflate(d / "full.gz")
    first = b"Genomes joined: %d from p1.gz, the index holds %d\n" % (sizes["p1"], sizes["p0"] + sizes["p1"])
    second = b"Genomes joined: %d from b.gz, the index holds %d\n" % (sizes["b"], sizes["full"])
    assert first in so and second in so and so.index(first) < so.index(second)


@pytest.mark.parametrize("name", ["messy", "w16"])
def test_queries_and_representatives_after_a_join(workdirs, name):
    d = workdirs(name).need("full", "a", "b").d
    cli(["-i", "full.gz", "-X", "-n", "0", "-o", "x_full.txt", "-t", "1"], d)
    cli(["-i", "a.gz", "-M", "b.gz", "-X", "-n", "0", "-o", "x.txt", "-t", "1"], d)
    want = (d / "x_full.txt").read_bytes()
    assert want.count(b"\n") >= 2
    assert (d / "x.txt").read_bytes() == want
    cli(["-i", "full.gz", "-R", "reps_full.txt", "-o", "r1.txt", "-t", "1"], d)
    cli(["-i", "a.gz", "-M", "b.gz", "-R", "reps.txt", "-o", "r2.txt", "-t", "1"], d)
    want = (d / "reps_full.txt").read_bytes()
    assert want.strip()
    assert (d / "reps.txt").read_bytes() == want


def test_a_reference_written_file_joined_with_itself(golden_dir, tmp_path):
    """the reference's own -d output: its columns are inflated on the host, the other load path"""
    ref_idx = os.path.join(golden_dir, "rnd3_ref_idx.gz")
    G = genomes_of(ref_idx)
    so = cli(["-i", ref_idx, "-M", ref_idx, "-d", "twice.gz", "-o", "o.txt", "-t", "1"], tmp_path).stdout
    assert b"Genomes joined: %d from %s, the index holds %d\n" % (G, ref_idx.encode(), 2 * G) in so
    one = np.frombuffer(inflate(ref_idx, also=(38,)), np.uint8)       # (38: the compressed flag)
    assert inflate(tmp_path / "twice.gz", also=(38,)) == extend_ref.joined_stream(one, one).tobytes()


def test_join_is_refused_before_any_work(workdirs):
    w = workdirs("messy").need("a", "b")
    case, d, base = w.case, w.d, w.base
    assert base[2] == "-h"
    other = base[:3] + [str(case.h - 1)] + base[4:]
    cli(["-l", "b.lst", "-d", "b_other_h.gz", "-o", "build_other.txt", *other], d)
    for args, env, devices, msg in (
            (["-l", "a.lst", *base, "-M", "b.gz"], {}, "0", b"-M is not supported with -l"),
            (["-i", "a.gz", "-M", "b.gz"], {}, "0,0", b"-M is not supported with several GPUs"),
            (["-i", "a.gz", "-M", "b.gz"], {"WORLD_SIZE": "2", "RANK": "0"}, "0", b"-M is not supported with one process per GPU"),
            (["-i", "a.gz", "-M", "b.gz", "-M", "b_other_h.gz"], {}, "0", b"different parameters: -h differs"),
            (["-i", "a.gz", "-M", "b.gz", "-M", "nowhere.gz"], {}, "0", b"-M: cannot read nowhere.gz")):
        r = cli([*args, "-d", "never.gz", "-o", "never.txt", "-t", "1"], d, devices=devices, env=env, ok=False)
        assert r.returncode == 1 and msg in r.stdout, (args, r.stdout)
        assert b"Genomes joined" not in r.stdout
        assert not (d / "never.gz").exists() and not (d / "never.txt").exists()
