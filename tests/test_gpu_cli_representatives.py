"""`miekki -R <file> -r <file>`: the representatives of the indexed genomes at -X's thresholds -- a list -K takes -- and the
clusters around them in -F's layout.  The yardstick is the oracle's rows through tests/representatives_ref.py: the files'
bytes and the stdout line are what its answer formats to."""
import gzip

import numpy as np
import pytest

import families_ref as fr
import representatives_ref as rr
import synth
from cli_util import cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdirs(tmp_path_factory):
    """a case's files, list and dumped index, and the model's answer for its genomes at min_score 10, 0.5 * threshold"""
    dirs = {}

    def get(name):
        if name not in dirs:
            case = (synth.CASES.get(name) or synth.EXTRA_CASES[name])()
            d = tmp_path_factory.mktemp(name)
            for fn, data, gz in dict((f[0], f) for f in case.genome_files).values():
                (d / fn).write_bytes(gzip.compress(data, 1) if gz else data)
            (d / "genomes.lst").write_bytes(b"".join(fn.encode() + b"\n" for fn, _, _ in case.genome_files))
            base = ["-k", str(case.k), "-h", str(case.h), "-f", str(case.f), "-b", str(case.b), "-s", str(case.threshold), "-t", "1"]
            cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "o.txt", *base], d)
            a = fr.Answer((case.k, case.h, case.fp_bits, case.b, case.threshold), case.genome_sequences())
            dirs[name] = (d, base, rr.representatives(a))
        return dirs[name]
    return get


@pytest.mark.parametrize("name", ["messy", "dups"])
def test_representative_and_cluster_files_and_summary(workdirs, name):
    d, base, rep = workdirs(name)
    so = cli(["-i", "full.gz", "-R", "reps.txt", "-r", "clusters.txt", "-o", "oi.txt", "-t", "1"], d).stdout
    assert (d / "reps.txt").read_bytes() == rr.format_representatives(rep)
    assert (d / "clusters.txt").read_bytes() == fr.format_labels(rep)
    assert rr.summary_line(rep) + b"\n" in so
    # either flag alone, -r while the index is built from the list and beside a query flag
    so = cli(["-l", "genomes.lst", "-r", "clusters_l.txt", "-X", "-o", "ol.txt", *base], d).stdout
    assert (d / "clusters_l.txt").read_bytes() == fr.format_labels(rep) and rr.summary_line(rep) + b"\n" in so


def test_representatives_file_is_a_keep_list(workdirs):
    """-R, then -K with that file and -d, then -R over the smaller index: every genome its own representative"""
    d, base, rep = workdirs("rnd3")
    n = int((rep == np.arange(len(rep))).sum())
    assert 1 < n < len(rep)                                                              # (on the oracle: something is dropped)
    cli(["-i", "full.gz", "-R", "reps.txt", "-o", "o1.txt", "-t", "1"], d)
    assert (d / "reps.txt").read_bytes() == rr.format_representatives(rep)
    cli(["-i", "full.gz", "-K", "reps.txt", "-d", "small.gz", "-o", "o2.txt", "-t", "1"], d)
    so = cli(["-i", "small.gz", "-R", "again.txt", "-o", "o3.txt", "-t", "1"], d).stdout
    assert (d / "again.txt").read_bytes() == b"".join(b"%d\n" % j for j in range(n))
    assert b"representatives: %d of %d, largest cluster 1\n" % (n, n) in so


@pytest.mark.parametrize("flag", ["-R", "-r"])
def test_refused_with_several_contexts_or_one_process_per_gpu(tmp_path, flag):
    r = cli(["-l", "genomes.lst", flag, "reps.txt"], tmp_path, devices="0,0", ok=False)
    assert r.returncode == 1 and b"-R / -r are not supported with several GPUs in the process" in r.stdout
    assert r.stdout.count(b"\n") == 1
    assert b"Using " not in r.stdout and not (tmp_path / "out.txt").exists() and not (tmp_path / "reps.txt").exists()
    r = cli(["-l", "genomes.lst", flag, "reps.txt"], tmp_path, env={"MIEKKI_RANK": "0", "MIEKKI_WORLD": "2"}, ok=False)
    assert r.returncode == 1 and b"-R / -r are not supported with one process per GPU" in r.stdout
    assert r.stdout.count(b"\n") == 1
    assert b"Using " not in r.stdout and not (tmp_path / "out.txt").exists() and not (tmp_path / "reps.txt").exists()
