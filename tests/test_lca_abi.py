"""The lowest-common-ancestor entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the
library, bound in miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  The reader
of `miekki -T`'s file and the writers of -y and -Y (host/taxonomy.hpp) under AddressSanitizer + UBSan, as a stand-alone
program.  And the command line's refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lca_ref as lr
from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "miekki_amd", "miekki")
CTX, TAX, LT = r"mk_ctx\s*\*\s*\w*", r"const\s+mk_taxonomy\s*\*\s*\w+", r"mk_lca_tally\s*\*\s*\w+"
U32, DBL, CU32P, U32P = r"uint32_t\s+\w+", r"double\s+\w+", r"const\s+uint32_t\s*\*\s*\w+", r"uint32_t\s*\*\s*\w+"
SEQS = r"const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+"
CALLS = {
    "mk_taxonomy_create": rf"int\s+mk_taxonomy_create\s*\(\s*{CTX},\s*{CU32P},\s*{CU32P},\s*{U32},\s*{U32},\s*mk_taxonomy\s*\*\s*\*\s*\w+\s*\)",
    "mk_taxonomy_nodes": rf"uint32_t\s+mk_taxonomy_nodes\s*\(\s*{TAX}\s*\)",
    "mk_taxonomy_parents": rf"int\s+mk_taxonomy_parents\s*\(\s*{TAX},\s*{U32P}\s*\)",
    "mk_taxonomy_free": rf"void\s+mk_taxonomy_free\s*\(\s*{CTX},\s*mk_taxonomy\s*\*\s*\w+\s*\)",
    "mk_lca_tally_reset": rf"int\s+mk_lca_tally_reset\s*\(\s*{CTX},\s*{LT},\s*{U32}\s*\)",
    "mk_qset_run_lca": rf"int\s+mk_qset_run_lca\s*\(\s*{CTX},\s*mk_qset\s*\*\s*\w+,\s*{U32},\s*{DBL},\s*{U32},\s*{TAX},\s*{LT},\s*{U32},\s*{U32P}\s*\)",
    "mk_lca_tally_read": rf"int\s+mk_lca_tally_read\s*\(\s*{CTX},\s*const\s+{LT},\s*{U32},\s*{LT}\s*\)",
    "mk_query_lca": rf"int\s+mk_query_lca\s*\(\s*{CTX},\s*{SEQS},\s*{U32},\s*{U32},\s*{DBL},\s*{U32},\s*{CU32P},\s*{CU32P},\s*{U32},\s*{LT},\s*{U32P}\s*\)",
}


def test_header_declares_and_library_exports_the_lca_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert [L.SIGNATURES[n][0] for n in CALLS] == [L.i32, L.u32, L.i32, None, L.i32, L.i32, L.i32, L.i32]
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+reads\s*,\s*best_matches\s*,\s*hits\s*;\s*\}\s*mk_lca_tally\s*;", text)
    assert re.search(r"typedef\s+struct\s+mk_taxonomy\s+mk_taxonomy\s*;", text)
    assert re.search(r"#define\s+MK_NO_NODE\s+0xffffffffu\b", text) and L.NO_NODE == 0xffffffff
    assert re.search(r"#define\s+MK_LCA_ABOVE\s+0xfffffffeu\b", text) and L.LCA_ABOVE == 0xfffffffe
    run = L.SIGNATURES["mk_qset_run_lca"][1]
    assert len(run) == 9 and run[3] is ctypes.c_double and run[4] is L.u32
    one = L.SIGNATURES["mk_query_lca"][1]
    assert len(one) == 12 and one[5] is ctypes.c_double
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert (ctypes.sizeof(L.Tally), ctypes.sizeof(L.CladeTally), ctypes.sizeof(L.Depth), ctypes.sizeof(L.Pick)) == (32, 40, 16, 24)
    assert ctypes.sizeof(L.LcaTally) == 24
    assert [f[0] for f in L.LcaTally._fields_] == ["reads", "best_matches", "hits"]
    assert all(f[1] is ctypes.c_uint64 for f in L.LcaTally._fields_)


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    out = ctypes.c_void_p()
    lo, hi = (ctypes.c_uint32 * 2)(0, 0), (ctypes.c_uint32 * 2)(4, 2)
    for status in (lib.mk_taxonomy_create(None, lo, hi, 2, 4, ctypes.byref(out)),
                   lib.mk_taxonomy_parents(None, lo),
                   lib.mk_lca_tally_reset(None, None, 4),
                   lib.mk_qset_run_lca(None, None, 10, 1.0, 100, None, None, 4, None),
                   lib.mk_lca_tally_read(None, None, 4, None),
                   lib.mk_query_lca(None, None, None, 4, 10, 1.0, 100, lo, hi, 2, None, None)):
        assert status == -1
        assert b"null argument" in lib.mk_last_error()
    assert out.value is None
    assert lib.mk_taxonomy_nodes(None) == 0
    lib.mk_taxonomy_free(None, None)                                       # nothing to free: nothing happens


def test_python_has_lca():
    from miekki_amd.index import Miekki
    assert callable(Miekki.lca)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("taxonomy_check")
    exe = str(d / "taxonomy_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "taxonomy_check.cpp")], check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], cwd=d, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
        return r.stdout
    return d, run


BAD = {
    "overlap.txt": (b"0 99\n10 19\n\n15 30 x\n", b"line 4 of overlap.txt", b"overlaps"),
    "twice.txt": (b"# t\n0 99\n10 19\n10 19 again\n", b"line 4 of twice.txt", b"repeats"),
    "child_first.txt": (b"10 19\n10 30\n", b"line 2 of child_first.txt", b"preorder"),
    "back.txt": (b"0 99\n10 19\n5 8\n", b"line 3 of back.txt", b"preorder"),
    "reversed.txt": (b"0 99\n19 10\n", b"line 2 of reversed.txt", b"below the first"),
    "words.txt": (b"0 99\n10 nineteen\n", b"line 2 of words.txt", b"is not a node"),
    "one_id.txt": (b"0 99\n\n10\n", b"line 3 of one_id.txt", b"is not a node"),
    "glued.txt": (b"0 99x\n", b"line 1 of glued.txt", b"is not a node"),
    "huge.txt": (b"0 99999999999\n", b"line 1 of huge.txt", b"is not a node"),
}


def test_taxonomy_files_under_sanitizers(checker):
    """the five layouts are read as lca_ref derives them; what is no taxonomy is refused, the line named; the report, the
    per-read lines and the summary are lca_ref's bytes"""
    d, run = checker
    for name, nodes in lr.taxonomies().items():
        tree, names = lr.Tree(nodes, 1101), lr.names_of(nodes)
        text = lr.taxonomy_file(nodes, names)
        (d / f"{name}.txt").write_bytes(text)
        out = run("parse", f"{name}.txt").split(b"\n")
        assert out[0] == b"ok %d" % len(nodes), out[0]
        lines = [i + 1 for i, l in enumerate(text.split(b"\n")) if l and not l.startswith(b"#")]
        for v, (lo, hi) in enumerate(nodes):
            p = tree.parent[v]
            assert out[1 + v] == b"%d %d %d %d %d |%s|" % (lo, hi, -1 if p is None else p, tree.depth[v], lines[v], names[v].encode()), (name, v)
        assert run("fits", f"{name}.txt", 1101) == b"ok\n"
        if nodes:
            assert b"refused: -T: line " in run("fits", f"{name}.txt", 1100) and b"genome id 1100 is beyond the index's 1100 genomes" in run("fits", f"{name}.txt", 1100)
        rng = np.random.default_rng(len(nodes))
        counts = rng.integers(0, 1000, (len(nodes) + 1, 3)).astype(np.uint64) * (rng.random((len(nodes) + 1, 1)) < 0.3)
        counts = counts.astype(np.uint64)
        (d / "counts.txt").write_text("\n".join(" ".join(str(int(x)) for x in r) for r in counts))
        assert run("report", f"{name}.txt", "counts.txt") == lr.format_report(counts, tree, names) + lr.summary_line(counts, 99, 10) + b"\n", name
    (d / "crlf.txt").write_bytes(b"0 9 root \r\n  2\t 3  a  b \r\n")
    assert run("parse", "crlf.txt") == b"ok 2\n0 10 -1 0 1 |root|\n2 4 0 1 2 |a  b|\n"
    (d / "none.txt").write_bytes(b"# nothing\n\n")
    assert run("parse", "none.txt") == b"ok 0\n"
    for name, (text, line, says) in BAD.items():
        (d / name).write_bytes(text)
        out = run("parse", name)
        assert out.startswith(b"refused: -T: ") and line in out and says in out, out
    assert run("reads", 3, "*", "-", 0) == lr.format_reads(np.array([0] * 7 + [3, lr.ABOVE, lr.NO_NODE, 0], np.uint32)).split(b"\n", 7)[7]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lca_cli")
    (d / "good.txt").write_bytes(b"0 3 root\n0 1\n")
    for name, (text, _, _) in BAD.items():
        (d / name).write_bytes(text)
    (d / "reads.fa").write_bytes(b">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    (d / "list.txt").write_bytes(b"reads.fa\n")
    (d / "index.gz").write_bytes(b"not looked at")
    return d


REFUSALS = [
    (["-i", "index.gz", "-a", "reads.fa", "-y", "no.txt"], b"it needs -T"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt"], b"it needs -y"),
    (["-i", "index.gz", "-a", "reads.fa", "-Y", "no.txt"], b"-Y receives every read's node of a taxonomy: it needs -T"),
    (["-i", "index.gz", "-a", "reads.fa", "-P", "no.txt", "-m", "10"], b"-m is the margin of the placement in a taxonomy: it needs -T"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-m", "101"], b"-m takes a percentage"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-m", "-1"], b"-m takes a percentage"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-m", "ten"], b"-m takes a percentage"),
    (["-i", "index.gz", "-T", "good.txt", "-y", "no.txt"], b"it needs -a"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-e"], b"-y"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-A", "reads.fa"], b"-y"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-X"], b"-y"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-n", "5"], b"it takes no -n"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "good.txt", "-y", "no.txt", "-S", "list.txt", "-c", "no_c.txt"], b"-S"),
    (["-i", "index.gz", "-a", "reads.fa", "-T", "no_such_file.txt", "-y", "no.txt"], b"-T: cannot read no_such_file.txt"),
] + [(["-i", "index.gz", "-a", "reads.fa", "-T", name, "-y", "no.txt"], line) for name, (_, line, _) in BAD.items()]


@pytest.mark.parametrize("args,says", REFUSALS)
def test_refusals_before_any_device(files, args, says):
    """exit status 1, the flag named, no "Using " line -- no device was touched -- and nothing written"""
    e = dict(os.environ, MIEKKI_DEVICES="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK"):
        e.pop(k, None)
    before = sorted(os.listdir(files))
    r = subprocess.run([CLI, *args, "-o", "no_out.txt"], cwd=files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert r.returncode == 1, r.stdout
    assert says in r.stdout
    assert b"Using " not in r.stdout
    assert sorted(os.listdir(files)) == before


def test_usage_names_the_flags():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0
    for flag in (b"  -T <file>", b"  -y <file>", b"  -Y <file>", b"  -m <int>"):
        assert flag in r.stdout
