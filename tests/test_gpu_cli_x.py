"""`miekki -X`: every indexed genome against the index, from its stored column.  The yardstick is the real reference: its
own -A output over the SAME files (tests/golden/<case>_outA.txt, where qfiles.lst is the indexed list) -- a genome's file
queried as a whole is the genome's column queried (tests/test_stored_column_is_the_query.py)."""
import gzip
import os

import pytest

import synth
from cli_util import cli

pytestmark = pytest.mark.gpu
CASES = ["messy", "h20", "w16", "c1", "c2mini", "h16z", "rnd0", "rnd1", "rnd2", "rnd3", "rnd4", "rnd5"]


@pytest.fixture(scope="module")
def workdirs(tmp_path_factory):
    dirs = {}

    def get(name):
        if name not in dirs:
            case = (synth.CASES.get(name) or synth.EXTRA_CASES[name])()
            d = tmp_path_factory.mktemp(name)
            for fn, data, gz in dict((f[0], f) for f in case.genome_files).values():     # (a file may be listed many times)
                (d / fn).write_bytes(gzip.compress(data, 1) if gz else data)
            (d / "genomes.lst").write_bytes(b"".join(fn.encode() + b"\n" for fn, _, _ in case.genome_files)
                                            + b"missing_file.fa\nab\n")
            base = ["-k", str(case.k), "-h", str(case.h), "-f", str(case.f), "-b", str(case.b),
                    "-s", str(case.threshold), "-t", "1"]
            dirs[name] = (case, d, base)
        return dirs[name]
    return get


def golden_outA(golden_dir, name):
    return open(os.path.join(golden_dir, f"{name}_outA.txt"), "rb").read()


@pytest.mark.parametrize("name", CASES)
def test_x_after_l_is_the_reference_querying_the_same_files(workdirs, golden_dir, name):
    case, d, base = workdirs(name)
    so = cli(["-l", "genomes.lst", "-X", "-o", "outX.txt", "-d", "idx.gz", *base], d).stdout
    assert (d / "outX.txt").read_bytes() == golden_outA(golden_dir, name)
    assert b"running in approx mode, intersection is estimated by the index" in so and b"The end" in so
    # after -i there are no names: the same lines, the genome's id in their place.  Kept files (sequence >= k) have ids in
    # list order; a file listed twice has the same line twice, so looking lines up by name is unambiguous.
    lines = dict(ln.split(b":", 1) for ln in golden_outA(golden_dir, name).splitlines(keepends=True))
    kept = [fn for fn, data, _ in case.genome_files
            if len(b"".join(l for l in data.split(b"\n") if not l.startswith(b">"))) >= case.k]
    want = b"".join(b"%d:" % g + lines[fn.encode()] for g, fn in enumerate(kept) if fn.encode() in lines)
    cli(["-i", "idx.gz", "-X", "-o", "outX_i.txt", "-t", "1"], d)
    assert (d / "outX_i.txt").read_bytes() == want


@pytest.mark.parametrize("name", ["messy", "w16", "rnd1"])
def test_x_over_three_shards(workdirs, golden_dir, name):
    """the owner's columns exported on its GPU, copied to the others, sets from columns there: one context's bytes"""
    case, d, base = workdirs(name)
    cli(["-l", "genomes.lst", "-X", "-o", "outX_m.txt", *base], d, devices="0,0,0")
    assert (d / "outX_m.txt").read_bytes() == golden_outA(golden_dir, name)


def test_x_on_the_tie_heavy_collection(workdirs):
    """`dups`: every genome above the thresholds (-n 0) over two shards, and the reference's ten where every entrant row
    overflows -- rerun with wide rows, and (MIEKKI_SHARD_WIDE_ROWS=0) answered from dense score rows of the prepared sets"""
    case, d, base = workdirs("dups")
    cli(["-l", "genomes.lst", "-X", "-n", "0", "-o", "all_1.txt", *base], d)
    one = (d / "all_1.txt").read_bytes()
    assert one.count(b"\n") == 304 and min(ln.count(b";") for ln in one.splitlines()[1:50]) >= 300     # (every copy finds every copy)
    cli(["-l", "genomes.lst", "-X", "-n", "0", "-o", "all_2.txt", *base], d, devices="0,0")
    assert (d / "all_2.txt").read_bytes() == one
    cli(["-l", "genomes.lst", "-X", "-o", "ten_1.txt", *base], d)
    ten = (d / "ten_1.txt").read_bytes()
    assert ten.count(b"\n") == 304
    for i, wide in enumerate(("1", "0")):
        cli(["-l", "genomes.lst", "-X", "-o", f"ten_2{i}.txt", *base], d, devices="0,0", env={"MIEKKI_SHARD_WIDE_ROWS": wide})
        assert (d / f"ten_2{i}.txt").read_bytes() == ten


@pytest.mark.parametrize("name", ["dups", "messy"])
@pytest.mark.parametrize("N", [3, 100])
def test_x_with_a_finite_n_over_two_shards(workdirs, name, N):
    """-n 3: the shards' entrant rows merged on the first GPU (`dups`: every row overflows); -n 100: the shards' candidate
    lists under one heap of 100.  One context's bytes either way."""
    case, d, base = workdirs(name)
    cli(["-l", "genomes.lst", "-X", "-n", str(N), "-o", f"n{N}_1.txt", *base], d)
    one = (d / f"n{N}_1.txt").read_bytes()
    assert one.count(b"\n") >= 3 and max(ln.count(b";") for ln in one.splitlines()) >= min(N, 3)
    cli(["-l", "genomes.lst", "-X", "-n", str(N), "-o", f"n{N}_2.txt", *base], d, devices="0,0")
    assert (d / f"n{N}_2.txt").read_bytes() == one


@pytest.mark.parametrize("args,env,msg", [
    (["-X", "-e"], {}, b"-X queries the indexed genomes themselves"),
    (["-X", "-a", "q.fa"], {}, b"-X queries the indexed genomes themselves"),
    (["-X", "-A", "q.lst"], {}, b"-X queries the indexed genomes themselves"),
    (["-X"], {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}, b"-X is not supported with one process per GPU"),
])
def test_x_is_refused_before_any_work(tmp_path, args, env, msg):
    r = cli(["-l", "genomes.lst", *args], tmp_path, env=env, ok=False)
    assert r.returncode == 1 and msg in r.stdout
    assert b"Using " not in r.stdout and not (tmp_path / "out.txt").exists()
