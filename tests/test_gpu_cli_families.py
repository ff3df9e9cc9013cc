"""`miekki -F <file>`: the families of the indexed genomes at -X's thresholds, as a list -K takes.  The yardstick is the
oracle's rows through tests/families_ref.py: the file's bytes and the stdout line are what its labels format to."""
import gzip

import numpy as np
import pytest

import families_ref as fr
import synth
from cli_util import cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def workdirs(tmp_path_factory):
    """a case's files and list, and the oracle's labels of its genomes at min_score 10, 0.5 * threshold"""
    dirs = {}

    def get(name):
        if name not in dirs:
            case = (synth.CASES.get(name) or synth.EXTRA_CASES[name])()
            d = tmp_path_factory.mktemp(name)
            for fn, data, gz in dict((f[0], f) for f in case.genome_files).values():
                (d / fn).write_bytes(gzip.compress(data, 1) if gz else data)
            (d / "genomes.lst").write_bytes(b"".join(fn.encode() + b"\n" for fn, _, _ in case.genome_files))
            base = ["-k", str(case.k), "-h", str(case.h), "-f", str(case.f), "-b", str(case.b), "-s", str(case.threshold), "-t", "1"]
            a = fr.Answer((case.k, case.h, case.fp_bits, case.b, case.threshold), case.genome_sequences())
            dirs[name] = (d, base, a.labels())
        return dirs[name]
    return get


@pytest.mark.parametrize("name", ["messy", "dups", "rnd3"])
def test_family_file_and_summary(workdirs, name):
    d, base, labels = workdirs(name)
    want = fr.format_labels(labels)
    so = cli(["-l", "genomes.lst", "-F", "fam.txt", "-d", "full.gz", "-o", "o.txt", *base], d).stdout
    assert (d / "fam.txt").read_bytes() == want
    assert fr.summary_line(labels) + b"\n" in so
    # three contexts: a forest per shard, folded on the first
    so3 = cli(["-l", "genomes.lst", "-F", "fam3.txt", "-o", "o3.txt", *base], d, devices="0,0,0").stdout
    assert (d / "fam3.txt").read_bytes() == want and fr.summary_line(labels) + b"\n" in so3
    # from the dumped index, with and without a query flag beside it
    cli(["-i", "full.gz", "-F", "fam_i.txt", "-o", "oi.txt", "-t", "1"], d)
    assert (d / "fam_i.txt").read_bytes() == want
    cli(["-i", "full.gz", "-F", "fam_x.txt", "-X", "-o", "ox.txt", "-t", "1"], d, devices="0,0,0")
    assert (d / "fam_x.txt").read_bytes() == want


def test_family_file_is_a_keep_list(workdirs):
    """-F, then -K with that file, then -d: the dump Miekki.select writes for the same order, families side by side"""
    import miekki_amd
    d, base, labels = workdirs("rnd3")
    assert len(set(labels)) > 1 and list(np.argsort(labels, kind="stable")) != list(range(len(labels)))   # (the order changes)
    cli(["-l", "genomes.lst", "-F", "fam.txt", "-d", "full.gz", "-o", "o.txt", *base], d)
    cli(["-i", "full.gz", "-K", "fam.txt", "-d", "grouped.gz", "-F", "fam2.txt", "-o", "o2.txt", "-t", "1"], d)
    order = [int(x) for x in (d / "fam.txt").read_text().split()]
    assert order == [int(g) for g in np.argsort(labels, kind="stable")]
    ix = miekki_amd.Miekki.load(str(d / "full.gz"))
    try:
        ix.select(order)
        ix.dump_disk(str(d / "select.gz"))
    finally:
        ix.close()

    def stream(path):
        raw = bytearray(gzip.open(path, "rb").read())
        raw[32] = 0
        return bytes(raw)
    assert stream(d / "grouped.gz") == stream(d / "select.gz")
    # after -K every family is a run of consecutive ids
    moved = [int(l) for l in labels[order]]
    assert (d / "fam2.txt").read_bytes() == fr.format_labels([moved.index(l) for l in moved])
    assert [int(x) for x in (d / "fam2.txt").read_text().split()] == list(range(len(labels)))


def test_families_are_refused_with_one_process_per_gpu(tmp_path):
    r = cli(["-l", "genomes.lst", "-F", "fam.txt"], tmp_path, env={"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}, ok=False)
    assert r.returncode == 1 and b"-F is not supported with one process per GPU" in r.stdout
    assert b"Using " not in r.stdout and not (tmp_path / "out.txt").exists() and not (tmp_path / "fam.txt").exists()
