"""The marker entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library, bound
in miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  The writer of `miekki -V`
(host/taxonomy.hpp) under AddressSanitizer + UBSan, as a stand-alone program.  And the command line's refusals that need no
device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lca_ref as lr
import markers_ref as mr
from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "miekki_amd", "miekki")
CTX, TAX, NM = r"mk_ctx\s*\*\s*\w*", r"const\s+mk_taxonomy\s*\*\s*\w+", r"mk_node_markers\s*\*\s*\w+"
U32, CU32P, U64P = r"uint32_t\s+\w+", r"const\s+uint32_t\s*\*\s*\w+", r"uint64_t\s*\*\s*\w+"
SEQS = r"const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+"
CALLS = {
    "mk_taxonomy_markers": rf"int\s+mk_taxonomy_markers\s*\(\s*{CTX},\s*{TAX},\s*{CU32P},\s*{NM},\s*{U32},\s*{U64P}\s*\)",
    "mk_query_taxonomy_markers": rf"int\s+mk_query_taxonomy_markers\s*\(\s*{CTX},\s*{SEQS},\s*{U32},\s*{CU32P},\s*{CU32P},\s*{U32},\s*{NM},\s*{U32},\s*{U64P}\s*\)",
}


def test_header_declares_and_library_exports_the_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+specific\s*,\s*covered\s*;\s*\}\s*mk_node_markers\s*;", text)
    assert L.SIGNATURES["mk_taxonomy_markers"] == (L.i32, [L.vp, L.vp, L.vp, L.vp, L.u32, L.vp])
    one = L.SIGNATURES["mk_query_taxonomy_markers"]
    assert one[0] is L.i32 and len(one[1]) == 10 and [i for i, t in enumerate(one[1]) if t is L.u32] == [3, 6, 8]
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert (ctypes.sizeof(L.Tally), ctypes.sizeof(L.CladeTally), ctypes.sizeof(L.Depth), ctypes.sizeof(L.Pick)) == (32, 40, 16, 24)
    assert (ctypes.sizeof(L.LcaTally), ctypes.sizeof(L.NodeCover)) == (24, 16)
    assert ctypes.sizeof(L.NodeMarkers) == 16
    assert [f[0] for f in L.NodeMarkers._fields_] == ["specific", "covered"]
    assert all(f[1] is ctypes.c_uint64 for f in L.NodeMarkers._fields_)


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    lo, hi = (ctypes.c_uint32 * 2)(0, 0), (ctypes.c_uint32 * 2)(4, 2)
    out, cells = (L.NodeMarkers * 3)(), ctypes.c_uint64(7)
    for r in out:
        r.specific, r.covered = 5, 6
    for status in (lib.mk_taxonomy_markers(None, None, None, out, 3, ctypes.byref(cells)),
                   lib.mk_query_taxonomy_markers(None, None, None, 4, lo, hi, 2, out, 3, ctypes.byref(cells))):
        assert status == -1
        assert b"null argument" in lib.mk_last_error()
    assert cells.value == 7 and all(r.specific == 5 and r.covered == 6 for r in out)


def test_python_has_markers():
    from miekki_amd.index import Miekki
    assert callable(Miekki.markers)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("markers_check")
    exe = str(d / "markers_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "markers_check.cpp")], check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], cwd=d, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
        return r.stdout
    return d, run


def test_the_writer_under_sanitizers(checker):
    """the file and the summary line are markers_ref's bytes: nodes without a covered cell in their subtree have no line, a
    node whose only covered cells lie below it has one, nodes without a name end in a tab, counters beyond 32 bits are
    written whole"""
    d, run = checker
    for name, nodes in lr.taxonomies().items():
        tree, names = lr.Tree(nodes, 1101), lr.names_of(nodes)
        (d / f"{name}.txt").write_bytes(lr.taxonomy_file(nodes, names))
        rng = np.random.default_rng(len(nodes) + 1)
        nm = np.zeros((len(nodes) + 1, 2), np.uint64)
        nm[:, 0] = rng.integers(1, 1 << 40, len(nodes) + 1)
        nm[:, 1] = (nm[:, 0] // np.uint64(3)) * (rng.random(len(nodes) + 1) < 0.4)
        if len(nodes):
            nm[0] = ((1 << 62) + 5, 0 if name == "deep" else (1 << 33) + 1)    # (`deep`: the root's line comes from below it)
        nm[-1] = ((1 << 35) + 9, (1 << 34) + 3)
        (d / "counts.txt").write_text("\n".join("%d %d" % (int(r[0]), int(r[1])) for r in nm))
        want = mr.format_markers(nm, tree, names) + mr.summary_line(99, nm, tree) + b"\n"
        assert run(f"{name}.txt", "counts.txt") == want, name
        if len(nodes) > 20:
            assert 1 < want.count(b"\n") < 1 + len(nodes)
        if name == "deep":
            assert want.startswith(b"0\t0\t0\t1100\t") and want.split(b"\n")[0].split(b"\t")[6:8] == [b"0", b"%d" % ((1 << 62) + 5)]
    assert run("empty.txt", "counts.txt").endswith(b"0 of 0 specific cells covered, 0 of 0 nodes covered, %d of %d cells above every node\n"
                                                   % ((1 << 34) + 3, (1 << 35) + 9))
    (d / "bad.txt").write_bytes(b"0 99\n10 19\n15 30 x\n")
    assert run("bad.txt", "counts.txt").startswith(b"refused: -T: line 3 of bad.txt")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("markers_cli")
    (d / "good.txt").write_bytes(b"0 3 root\n0 1\n")
    (d / "reads.fa").write_bytes(b">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    (d / "list.txt").write_bytes(b"reads.fa\n")
    (d / "index.gz").write_bytes(b"not looked at")
    return d


BASE = ["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-V", "no.txt"]
NO_LISTS = b"-V counts the cells the reads of -a hold per node that owns them: it takes no -e, -A or -X\n"
REFUSALS = [
    (["-i", "index.gz", "-a", "reads.fa", "-V", "no.txt"], b"-V credits every cell to the deepest node of a taxonomy that holds it: it needs -T\n"),
    (["-i", "index.gz", "-T", "good.txt", "-V", "no.txt"], b"-V screens the reads of a query file by the cells that belong to one node of a taxonomy: it needs -a\n"),
    (BASE + ["-e"], NO_LISTS),
    (BASE + ["-A", "list.txt"], NO_LISTS),
    (BASE + ["-X"], NO_LISTS),
    (BASE + ["-n", "5"], b"-V counts covered specific cells per node of the taxonomy, not hits per read: it takes no -n\n"),
    (BASE + ["-S", "list.txt", "-c", "no_c.txt"], b"-S takes its reads from the files of its list: it takes no -a, -A, -e or -X\n"),
    (["-i", "index.gz", "-T", "good.txt", "-V", "no.txt", "-S", "list.txt", "-c", "no_c.txt"],
     b"-V screens the reads of a query file by the cells that belong to one node of a taxonomy: it needs -a\n"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt"], b"-T names the taxonomy that -y reports the reads by: it needs -y\n"),
    (BASE + ["-Y", "no_reads.txt"], b"-Y receives every read's node of -y's placement: it needs -y\n"),
    (BASE + ["-m", "10"], b"-m is the margin of -y's placement: it needs -y\n"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "no_such_file.txt", "-V", "no.txt"], b"-T: cannot read no_such_file.txt\n"),
]


@pytest.mark.parametrize("args,says", REFUSALS)
def test_refusals_before_any_device(files, args, says):
    """exit status 1, the refusal the only output -- no "Using " line: no device was touched -- and nothing written"""
    e = dict(os.environ, MIEKKI_DEVICES="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK"):
        e.pop(k, None)
    before = sorted(os.listdir(files))
    r = subprocess.run([CLI, *args, "-o", "no_out.txt"], cwd=files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert r.returncode == 1, r.stdout
    assert r.stdout == says
    assert sorted(os.listdir(files)) == before


def test_several_gpus_and_ranks_are_refused(files):
    e = dict(os.environ, MIEKKI_DEVICES="0,1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK"):
        e.pop(k, None)
    before = sorted(os.listdir(files))
    r = subprocess.run([CLI, *BASE, "-o", "no_out.txt"], cwd=files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert r.returncode == 1
    assert r.stdout == b"-V is not supported with several GPUs in the process: the table of seen cells lives on one device (MIEKKI_DEVICES names one)\n"
    e = dict(e, MIEKKI_DEVICES="0", MIEKKI_WORLD="2", MIEKKI_RANK="0")
    r = subprocess.run([CLI, *BASE, "-o", "no_out.txt"], cwd=files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert r.returncode == 1 and r.stdout == b"-V is not supported with one process per GPU (MIEKKI_WORLD / WORLD_SIZE)\n"
    assert sorted(os.listdir(files)) == before


def test_usage_names_the_flag():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0
    assert b"  -V <file>  with -a and -T" in r.stdout and b"  -T <file>  with -y or -U" in r.stdout
