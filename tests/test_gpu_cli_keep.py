"""`miekki -K <file>`: keep the genomes the file lists, in its order, once the index exists and before -d and any query.
The yardstick for the dump is byte surgery with numpy on a file the existing -d path wrote: the header with the new
index_size, the kept columns, the kept sizes, the old Bloom filter (Miekki.cpp:649-719)."""
import gzip
import io
import struct

import numpy as np
import pytest

import synth
from cli_util import cli

pytestmark = pytest.mark.gpu
HDR = struct.Struct("<6IQBBIB")


@pytest.fixture(scope="module")
def workdirs(tmp_path_factory):
    """a case's files, its list, and full.gz = what `-l genomes.lst -d full.gz` writes"""
    dirs = {}

    def get(name):
        if name not in dirs:
            case = (synth.CASES.get(name) or synth.EXTRA_CASES[name])()
            d = tmp_path_factory.mktemp(name)
            for fn, data, gz in dict((f[0], f) for f in case.genome_files).values():
                (d / fn).write_bytes(gzip.compress(data, 1) if gz else data)
            (d / "genomes.lst").write_bytes(b"".join(fn.encode() + b"\n" for fn, _, _ in case.genome_files)
                                            + b"missing_file.fa\nab\n")
            base = ["-k", str(case.k), "-h", str(case.h), "-f", str(case.f), "-b", str(case.b),
                    "-s", str(case.threshold), "-t", "1"]
            cli(["-l", "genomes.lst", "-d", "full.gz", "-o", "build.txt", *base], d)
            kept = [fn for fn, data, _ in case.genome_files
                    if len(b"".join(l for l in data.split(b"\n") if not l.startswith(b">"))) >= case.k]
            dirs[name] = (case, d, base, kept)
        return dirs[name]
    return get


def inflate(path):
    raw = bytearray(gzip.open(path, "rb").read())
    raw[32] = 0
    return bytes(raw)


def cut(stream, ids):
    """the stream of the index that holds exactly the genomes `ids` of `stream`'s, under the same Bloom filter"""
    k, h, fpb, nbm, G, bl2, bbits, jac, cont, thr, comp = HDR.unpack(stream[:39])
    W, P = fpb // 8, 1 << h
    a = np.frombuffer(stream, np.uint8)
    o = 39
    cols = a[o:o + P * G * W].reshape(P, G, W); o += P * G * W
    gs = a[o:o + 8 * G].view(np.uint64); o += 8 * G
    bloom = a[o:o + bbits // 8]; o += bbits // 8
    ss = a[o:o + 4 * G].view(np.uint32); o += 4 * G
    assert o == len(a)
    ids = np.asarray(ids, np.int64)
    hdr = bytearray(HDR.pack(k, h, fpb, nbm, len(ids), bl2, bbits, jac, cont, thr, comp))
    hdr[32] = 0
    return b"".join([bytes(hdr), np.ascontiguousarray(cols[:, ids, :]).tobytes(), gs[ids].tobytes(), bloom.tobytes(), ss[ids].tobytes()])


def lists_for(G):
    assert G >= 4
    rng = np.random.default_rng(G)
    any_order = [G - 1, 0] + [int(g) for g in rng.permutation(np.arange(1, G - 1))[:max(1, (G - 2) * 2 // 3)]]
    ascending = [g for g in range(G) if g % 3 != 1]
    return any_order, ascending


def write_list(d, name, ids):
    (d / name).write_text("\n" + "".join(f"{g}\n\n" if i % 4 == 0 else f"{g}\n" for i, g in enumerate(ids)))


@pytest.mark.parametrize("name", ["messy", "w16"])
def test_dump_after_keep_is_the_cut_of_the_full_dump(workdirs, name):
    case, d, base, kept = workdirs(name)
    full = inflate(d / "full.gz")
    G = HDR.unpack(full[:39])[4]
    assert G == len(kept)
    any_order, ascending = lists_for(G)
    write_list(d, "keep.txt", any_order)
    so = cli(["-i", "full.gz", "-K", "keep.txt", "-d", "sub.gz", "-o", "o1.txt", "-t", "1"], d).stdout
    assert inflate(d / "sub.gz") == cut(full, any_order)
    assert b"Genomes kept: %d" % len(any_order) in so
    # three contexts: an ascending list is a pure subset of every shard; one that keeps only the last genomes empties shards
    write_list(d, "asc.txt", ascending)
    cli(["-i", "full.gz", "-K", "asc.txt", "-d", "sub3.gz", "-o", "o2.txt", "-t", "1"], d, devices="0,0,0")
    assert inflate(d / "sub3.gz") == cut(full, ascending)
    write_list(d, "tail.txt", [G - 2, G - 1])
    cli(["-i", "full.gz", "-K", "tail.txt", "-d", "tail.gz", "-X", "-o", "tailX3.txt", "-t", "1"], d, devices="0,0,0")
    assert inflate(d / "tail.gz") == cut(full, [G - 2, G - 1])
    cli(["-i", "full.gz", "-K", "tail.txt", "-X", "-o", "tailX1.txt", "-t", "1"], d)
    assert (d / "tailX3.txt").read_bytes() == (d / "tailX1.txt").read_bytes()
    # built and selected in one run: the same file as selecting the loaded one
    cli(["-l", "genomes.lst", "-K", "keep.txt", "-d", "sub_l.gz", "-o", "o3.txt", *base], d)
    assert inflate(d / "sub_l.gz") == cut(full, any_order)


@pytest.mark.parametrize("name", ["messy", "w16"])
def test_x_after_keep(workdirs, name):
    import miekki_amd
    case, d, base, kept = workdirs(name)
    full = inflate(d / "full.gz")
    G = HDR.unpack(full[:39])[4]
    any_order, ascending = lists_for(G)
    for fn, ids in (("keep.txt", any_order), ("asc.txt", ascending)):
        write_list(d, fn, ids)
        cli(["-i", "full.gz", "-K", fn, "-d", "s.gz", "-X", "-o", "x_i.txt", "-t", "1"], d)
        ix = miekki_amd.Miekki.load(str(d / "s.gz"))
        try:
            out = io.BytesIO()
            ix.query_index_file(out)
        finally:
            ix.close()
        want = out.getvalue()
        assert want.count(b"\n") >= 2
        assert (d / "x_i.txt").read_bytes() == want
        # after -l the lines carry the kept files' names, in the list's order
        named = b"".join(kept[ids[int(ln.split(b":", 1)[0])]].encode() + b":" + ln.split(b":", 1)[1]
                         for ln in want.splitlines(keepends=True))
        cli(["-l", "genomes.lst", "-K", fn, "-X", "-o", "x_l.txt", *base], d)
        assert (d / "x_l.txt").read_bytes() == named
    cli(["-l", "genomes.lst", "-K", "asc.txt", "-X", "-o", "x_l3.txt", *base], d, devices="0,0,0")
    assert (d / "x_l3.txt").read_bytes() == named
    cli(["-i", "full.gz", "-K", "asc.txt", "-X", "-o", "x_i3.txt", "-t", "1"], d, devices="0,0,0")
    assert (d / "x_i3.txt").read_bytes() == want


@pytest.mark.parametrize("text,devices,env,msg", [
    (None, "0", {}, b"-K: cannot read"),
    ("\n\n", "0", {}, b"lists no genome ids"),
    ("0\n1x\n", "0", {}, b"is not a genome id: 1x"),
    ("0\n-1\n", "0", {}, b"is not a genome id: -1"),
    ("2\n0\n2\n", "0", {}, b"genome id 2 is listed twice"),
    ("0\n1\n", "0", {"MIEKKI_RANK": "0", "MIEKKI_WORLD": "1"}, b"-K is not supported with one process per GPU"),
])
def test_keep_is_refused_before_any_work(tmp_path, text, devices, env, msg):
    if text is not None:
        (tmp_path / "keep.txt").write_text(text)
    r = cli(["-l", "genomes.lst", "-K", "keep.txt"], tmp_path, devices=devices, env=env, ok=False)
    assert r.returncode == 1 and msg in r.stdout
    assert b"Using " not in r.stdout and not (tmp_path / "out.txt").exists()


def test_keep_is_refused_once_the_index_is_known(workdirs):
    case, d, base, kept = workdirs("messy")
    G = len(kept)
    (d / "far.txt").write_text(f"0\n{G}\n1\n")
    for args in (["-i", "full.gz", "-t", "1"], ["-l", "genomes.lst", *base]):
        r = cli([*args, "-K", "far.txt", "-X", "-o", "never.txt", "-d", "never.gz"], d, ok=False)
        assert r.returncode == 1 and b"-K: genome id %d is not in the index" % G in r.stdout
        assert not (d / "never.txt").exists() and not (d / "never.gz").exists()
    (d / "desc.txt").write_text("3\n1\n")
    r = cli(["-i", "full.gz", "-t", "1", "-K", "desc.txt", "-X", "-o", "never.txt", "-d", "never.gz"], d, devices="0,0,0", ok=False)
    assert r.returncode == 1 and b"run it on one GPU" in r.stdout
    assert not (d / "never.txt").exists() and not (d / "never.gz").exists()
