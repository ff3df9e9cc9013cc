"""The abundance entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library,
bound in miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  The writer of
`miekki -E`'s file and line (host/abundance.hpp) under AddressSanitizer + UBSan, as a stand-alone program.  And the command
line's refusals that need no device."""
import ctypes
import os
import re
import subprocess

import pytest

import share_ref as sr
from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "miekki_amd", "miekki")
CTX, POOL, CPOOL = r"mk_ctx\s*\*\s*\w*", r"mk_sharepool\s*\*\s*\w+", r"const\s+mk_sharepool\s*\*\s*\w+"
U32, DBL, U64P, U32P = r"uint32_t\s+\w+", r"double\s+\w+", r"uint64_t\s*\*\s*\w+", r"uint32_t\s*\*\s*\w+"
CU64P, CU32P = r"const\s+uint64_t\s*\*\s*\w+", r"const\s+uint32_t\s*\*\s*\w+"
SEQS = r"const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+"
INFO, RES = r"mk_share_info\s*\*\s*\w+", r"mk_share_result\s*\*\s*\w+"
CALLS = {
    "mk_share_create": rf"int\s+mk_share_create\s*\(\s*{CTX},\s*mk_sharepool\s*\*\s*\*\s*\w+\s*\)",
    "mk_share_free": rf"void\s+mk_share_free\s*\(\s*{CTX},\s*{POOL}\s*\)",
    "mk_share_reset": rf"int\s+mk_share_reset\s*\(\s*{CTX},\s*{POOL}\s*\)",
    "mk_qset_run_share": rf"int\s+mk_qset_run_share\s*\(\s*{CTX},\s*mk_qset\s*\*\s*\w+,\s*{U32},\s*{DBL},\s*{U32},\s*{POOL}\s*\)",
    "mk_share_add_lists": rf"int\s+mk_share_add_lists\s*\(\s*{CTX},\s*{POOL},\s*{CU64P},\s*{CU32P},\s*{U32}\s*\)",
    "mk_share_info_read": rf"int\s+mk_share_info_read\s*\(\s*{CTX},\s*{CPOOL},\s*{INFO}\s*\)",
    "mk_share_export": rf"int\s+mk_share_export\s*\(\s*{CTX},\s*{CPOOL},\s*{U64P},\s*{U64P},\s*{U64P},\s*{U32P}\s*\)",
    "mk_share_rounds": rf"int\s+mk_share_rounds\s*\(\s*{CTX},\s*{POOL},\s*{U32},\s*{U32},\s*{U64P},\s*{RES}\s*\)",
    "mk_query_abundance": rf"int\s+mk_query_abundance\s*\(\s*{CTX},\s*{SEQS},\s*{U32},\s*{U32},\s*{DBL},\s*{U32},\s*{U32},\s*{U64P},\s*{U64P},\s*{U64P},\s*{INFO},\s*{RES}\s*\)",
}


def test_header_declares_and_library_exports_the_share_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert [L.SIGNATURES[n][0] for n in CALLS] == [L.i32, None, L.i32, L.i32, L.i32, L.i32, L.i32, L.i32, L.i32]
    assert re.search(r"typedef\s+struct\s+mk_sharepool\s+mk_sharepool\s*;", text)
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+queries\s*,\s*assigned\s*,\s*shared_reads\s*,\s*entries\s*;\s*\}\s*mk_share_info\s*;", text)
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+delta\s*,\s*starved\s*;\s*uint32_t\s+rounds\s*,\s*shift\s*;\s*\}\s*mk_share_result\s*;", text)
    assert re.search(r"#define\s+MK_SHARE_AUTO_SHIFT\s+0xffffffffu\b", text) and L.SHARE_AUTO_SHIFT == 0xffffffff
    run = L.SIGNATURES["mk_qset_run_share"][1]
    assert len(run) == 6 and run[3] is ctypes.c_double and run[4] is L.u32
    one = L.SIGNATURES["mk_query_abundance"][1]
    assert len(one) == 13 and one[5] is ctypes.c_double and one[6] is L.u32 and one[7] is L.u32
    assert len(L.SIGNATURES["mk_share_rounds"][1]) == 6 and len(L.SIGNATURES["mk_share_export"][1]) == 6
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert (ctypes.sizeof(L.Tally), ctypes.sizeof(L.CladeTally), ctypes.sizeof(L.LcaTally), ctypes.sizeof(L.Depth), ctypes.sizeof(L.Pick)) == (32, 40, 24, 16, 24)
    assert (ctypes.sizeof(L.ShareInfo), ctypes.sizeof(L.ShareResult)) == (32, 24)
    assert [f[0] for f in L.ShareInfo._fields_] == ["queries", "assigned", "shared_reads", "entries"]
    assert [f[0] for f in L.ShareResult._fields_] == ["delta", "starved", "rounds", "shift"]
    assert [f[1] for f in L.ShareResult._fields_] == [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    out = ctypes.c_void_p()
    off = (ctypes.c_uint64 * 2)(0, 0)
    info, res = L.ShareInfo(), L.ShareResult()
    for status in (lib.mk_share_create(None, ctypes.byref(out)),
                   lib.mk_share_reset(None, None),
                   lib.mk_qset_run_share(None, None, 10, 1.0, 100, None),
                   lib.mk_share_add_lists(None, None, off, None, 1),
                   lib.mk_share_info_read(None, None, ctypes.byref(info)),
                   lib.mk_share_export(None, None, None, None, None, None),
                   lib.mk_share_rounds(None, None, 1, 32, None, ctypes.byref(res)),
                   lib.mk_query_abundance(None, None, None, 4, 10, 1.0, 100, 5, None, None, None, None, ctypes.byref(res))):
        assert status == -1
        assert b"null argument" in lib.mk_last_error()
    assert out.value is None
    lib.mk_share_free(None, None)                                          # nothing to free: nothing happens


def test_python_has_abundance():
    from miekki_amd.index import Miekki
    assert callable(Miekki.abundance)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("abundance_check")
    exe = str(d / "abundance_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "abundance_check.cpp")], check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], cwd=d, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()[-2000:]
        return r.stdout
    return d, run


def test_abundance_file_under_sanitizers(checker):
    """the file and the line are share_ref's bytes: a pool small enough to follow, numbers at the ends of their ranges, nothing"""
    d, run = checker
    p = sr.Pool(9).add((0, 2)).add((2,)).add(()).add((0, 2, 4)).add((7, 8)).add((8,))
    for R, shift in ((1, None), (7, None), (7, 32)):
        A, delta, _, _ = sr.rounds(p, R, shift)
        (d / "counts.txt").write_text("".join("%d %d %d\n" % (A[g], p.unique[g], p.shared[g]) for g in range(p.G)))
        got = run("counts.txt", p.queries, p.assigned, len(p.lists), p.entries, R, 10, delta)
        assert got == sr.format_abundance(A, p.unique, p.shared) + sr.summary_line(p, R, 10, delta) + b"\n"
    top = 2 ** 64 - 1
    rows = [(top, top, 0), (0, 0, 0), ((2 ** 32 - 1) << 32, 0, top), (2 ** 32 - 1, 1, 1), (0, 0, 1)]
    (d / "edge.txt").write_text("".join("%d %d %d\n" % r for r in rows))
    got = run("edge.txt", top, top, top, top, 10000, 100, top)
    want = b"0\t4294967295.999\t%d\t0\n2\t4294967295.000\t0\t%d\n3\t0.999\t1\t1\n4\t0.000\t0\t1\n" % (top, top)
    assert want == sr.format_abundance([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert got == want + (b"abundance: %d queries, %d assigned, %d shared by several genomes, %d ids stored, 4 genomes listed, 10000 rounds, margin 100, "
                          b"last change 4294967295.999\n" % (top, top, top, top))
    (d / "none.txt").write_text("")
    assert run("none.txt", 0, 0, 0, 0, 50, 100, 0) == (b"abundance: 0 queries, 0 assigned, 0 shared by several genomes, 0 ids stored, 0 genomes listed, "
                                                      b"50 rounds, margin 100, last change 0.000\n")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("abundance_cli")
    (d / "reads.fa").write_bytes(b">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    (d / "list.txt").write_bytes(b"reads.fa\n")
    (d / "index.gz").write_bytes(b"not looked at")
    return d


BASE = ["-i", "index.gz", "-a", "reads.fa", "-E", "no.txt"]
HOW = b"-E splits the approximate mode's answers for the reads of -a among their genomes: it takes no -e, -A or -X\n"
REFUSALS = [
    (["-i", "index.gz", "-E", "no.txt"], b"-E estimates the abundances from the reads of a query file: it needs -a\n"),
    (BASE + ["-e"], HOW),
    (BASE + ["-A", "list.txt"], HOW),
    (BASE + ["-X"], HOW),
    (BASE + ["-n", "5"], b"-E reports reads per genome, not hits per read: it takes no -n\n"),
    (BASE + ["-S", "list.txt", "-c", "no_c.txt"], b"-S takes its reads from the files of its list: it takes no -a, -A, -e or -X\n"),
    (["-i", "index.gz", "-E", "no.txt", "-S", "list.txt", "-c", "no_c.txt"], b"-E estimates the abundances from the reads of a query file: it needs -a\n"),
    (["-i", "index.gz", "-a", "reads.fa", "-I", "7"], b"-I is the number of rounds of -E's estimate: it needs -E\n"),
    (["-i", "index.gz", "-a", "reads.fa", "-P", "no_p.txt", "-w", "10"], b"-w is the margin within which genomes share a read of -E's estimate: it needs -E\n"),
    (BASE + ["-I", "0"], b"-I takes a number of rounds, 1 .. 10000\n"),
    (BASE + ["-I", "10001"], b"-I takes a number of rounds, 1 .. 10000\n"),
    (BASE + ["-I", "-3"], b"-I takes a number of rounds, 1 .. 10000\n"),
    (BASE + ["-I", "seven"], b"-I takes a number of rounds, 1 .. 10000\n"),
    (BASE + ["-I", "7x"], b"-I takes a number of rounds, 1 .. 10000\n"),
    (BASE + ["-w", "101"], b"-w takes a percentage, 0 .. 100\n"),
    (BASE + ["-w", "-1"], b"-w takes a percentage, 0 .. 100\n"),
    (BASE + ["-w", "ten"], b"-w takes a percentage, 0 .. 100\n"),
    (BASE + ["-w", ""], b"-w takes a percentage, 0 .. 100\n"),
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
    r = subprocess.run([CLI, *BASE, "-o", "no_out.txt"], cwd=files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert r.returncode == 1 and r.stdout.startswith(b"-E is not supported with several GPUs in the process: the pool of shared reads lives on one device")
    e = dict(e, MIEKKI_DEVICES="0", MIEKKI_WORLD="2", MIEKKI_RANK="0")
    r = subprocess.run([CLI, *BASE, "-o", "no_out.txt"], cwd=files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert r.returncode == 1 and r.stdout.startswith(b"-E is not supported with one process per GPU")


def test_usage_names_the_flags():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0
    for flag in (b"  -E <file>", b"  -I <int>", b"  -w <int>"):
        assert flag in r.stdout
