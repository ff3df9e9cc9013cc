"""The clade tally entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library,
bound in miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  The reader of
`miekki -L`'s file and the writer of -p's (host/clades.hpp) under AddressSanitizer + UBSan, as a stand-alone program.  And the
command line's refusals that need no device."""
import ctypes
import os
import re
import subprocess

import pytest

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "miekki_amd", "miekki")
CTX, MAP, CT = r"mk_ctx\s*\*\s*\w*", r"const\s+mk_clade_map\s*\*\s*\w+", r"mk_clade_tally\s*\*\s*\w+"
U32, DBL = r"uint32_t\s+\w+", r"double\s+\w+"
SEQS = r"const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+"
CALLS = {
    "mk_clade_map_create": rf"int\s+mk_clade_map_create\s*\(\s*{CTX},\s*const\s+uint32_t\s*\*\s*\w+,\s*{U32},\s*mk_clade_map\s*\*\s*\*\s*\w+\s*\)",
    "mk_clade_map_size": rf"uint32_t\s+mk_clade_map_size\s*\(\s*{MAP}\s*\)",
    "mk_clade_map_free": rf"void\s+mk_clade_map_free\s*\(\s*{CTX},\s*mk_clade_map\s*\*\s*\w+\s*\)",
    "mk_clade_tally_reset": rf"int\s+mk_clade_tally_reset\s*\(\s*{CTX},\s*{CT},\s*{U32}\s*\)",
    "mk_qset_run_clade_tally": rf"int\s+mk_qset_run_clade_tally\s*\(\s*{CTX},\s*mk_qset\s*\*\s*\w+,\s*{U32},\s*{DBL},\s*{MAP},\s*{CT},\s*{U32},"
                               rf"\s*mk_tally\s*\*\s*\w+,\s*{U32}\s*\)",
    "mk_clade_tally_read": rf"int\s+mk_clade_tally_read\s*\(\s*{CTX},\s*const\s+{CT},\s*{U32},\s*{CT}\s*\)",
    "mk_query_clade_tally": rf"int\s+mk_query_clade_tally\s*\(\s*{CTX},\s*{SEQS},\s*{U32},\s*{U32},\s*{DBL},\s*const\s+uint32_t\s*\*\s*\w+,"
                            rf"\s*{U32},\s*{CT}\s*\)",
}


def test_header_declares_and_library_exports_the_clade_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    assert [L.SIGNATURES[n][0] for n in CALLS] == [L.i32, L.u32, None, L.i32, L.i32, L.i32, L.i32]
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+listed\s*,\s*unique\s*,\s*best\s*,\s*best_matches\s*,\s*hits\s*;\s*\}\s*mk_clade_tally\s*;", text)
    assert re.search(r"typedef\s+struct\s+mk_clade_map\s+mk_clade_map\s*;", text)
    assert re.search(r"#define\s+MK_NO_CLADE\s+0xffffffffu\b", text) and L.NO_CLADE == 0xffffffff
    run = L.SIGNATURES["mk_qset_run_clade_tally"][1]
    assert len(run) == 9 and run[3] is ctypes.c_double
    one = L.SIGNATURES["mk_query_clade_tally"][1]
    assert len(one) == 9 and one[5] is ctypes.c_double
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert (ctypes.sizeof(L.Tally), ctypes.sizeof(L.Depth), ctypes.sizeof(L.Pick)) == (32, 16, 24)
    assert ctypes.sizeof(L.CladeTally) == 40
    assert [f[0] for f in L.CladeTally._fields_] == ["listed", "unique", "best", "best_matches", "hits"]
    assert all(f[1] is ctypes.c_uint64 for f in L.CladeTally._fields_)


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    out = ctypes.c_void_p()
    numbers = (ctypes.c_uint32 * 4)(0, 0, 1, 1)
    for status in (lib.mk_clade_map_create(None, numbers, 4, ctypes.byref(out)),
                   lib.mk_clade_tally_reset(None, None, 4),
                   lib.mk_qset_run_clade_tally(None, None, 10, 1.0, None, None, 4, None, 0),
                   lib.mk_clade_tally_read(None, None, 4, None),
                   lib.mk_query_clade_tally(None, None, None, 4, 10, 1.0, None, 4, None)):
        assert status == -1
        assert b"null argument" in lib.mk_last_error()
    assert out.value is None
    assert lib.mk_clade_map_size(None) == 0
    lib.mk_clade_map_free(None, None)                                      # nothing to free: nothing happens


def test_python_has_clade_tally():
    from miekki_amd.index import Miekki
    assert callable(Miekki.clade_tally)


def test_clade_files_under_sanitizers(tmp_path):
    exe = str(tmp_path / "clades_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "clades_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1500


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("clade_cli")
    (d / "good.txt").write_bytes(b"0\n1\n\n2\n")
    (d / "unsorted.txt").write_bytes(b"0\n1\n\n3\n2\n")
    (d / "twice.txt").write_bytes(b"0\n1\n\n1\n")
    (d / "words.txt").write_bytes(b"0\none\n")
    (d / "empty.txt").write_bytes(b"\n\n")
    (d / "reads.fa").write_bytes(b">r\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    (d / "index.gz").write_bytes(b"not looked at")
    return d


@pytest.mark.parametrize("args,says", [
    (["-i", "index.gz", "-a", "reads.fa", "-p", "no.txt"], b"it needs -L"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "good.txt"], b"it needs -p"),
    (["-i", "index.gz", "-L", "good.txt", "-p", "no.txt"], b"it needs -a"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "good.txt", "-p", "no.txt", "-e"], b"-p"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "good.txt", "-p", "no.txt", "-A", "reads.fa"], b"-p"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "good.txt", "-p", "no.txt", "-X"], b"-p"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "good.txt", "-p", "no.txt", "-n", "5"], b"it takes no -n"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "unsorted.txt", "-p", "no.txt"], b"line 5 of unsorted.txt"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "twice.txt", "-p", "no.txt"], b"line 4 of twice.txt"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "words.txt", "-p", "no.txt"], b"line 2 of words.txt"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "empty.txt", "-p", "no.txt"], b"empty.txt lists no genome ids"),
    (["-i", "index.gz", "-a", "reads.fa", "-L", "no_such_file.txt", "-p", "no.txt"], b"-L: cannot read no_such_file.txt"),
])
def test_refusals_before_any_device(files, args, says):
    """exit status 1, the flag named, no "Using " line -- no device was touched -- and nothing written"""
    e = dict(os.environ, MIEKKI_DEVICES="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK"):
        e.pop(k, None)
    before = sorted(os.listdir(files))
    r = subprocess.run([CLI, *args, "-o", "no_out.txt"], cwd=files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=e)
    assert r.returncode == 1, r.stdout
    assert says in r.stdout and (b"-p" in r.stdout or b"-L" in r.stdout)
    assert b"Using " not in r.stdout
    assert sorted(os.listdir(files)) == before


def test_usage_names_both_flags():
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert r.returncode == 0 and b"  -L <file>" in r.stdout and b"  -p <file>" in r.stdout
