"""The tally entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library,
bound in miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  And the writer of
`miekki -P`'s file (host/profile.hpp) under AddressSanitizer + UBSan, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    "mk_tally_reset": r"int\s+mk_tally_reset\s*\(\s*mk_ctx\s*\*\s*\w*,\s*mk_tally\s*\*\s*\w+,\s*uint32_t\s+\w+\s*\)",
    "mk_qset_run_tally": r"int\s+mk_qset_run_tally\s*\(\s*mk_ctx\s*\*\s*\w*,\s*mk_qset\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*double\s+\w+,"
                         r"\s*mk_tally\s*\*\s*\w+,\s*uint32_t\s+\w+\s*\)",
    "mk_tally_read": r"int\s+mk_tally_read\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+mk_tally\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*mk_tally\s*\*\s*\w+\s*\)",
    "mk_query_tally": r"int\s+mk_query_tally\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+,"
                      r"\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*double\s+\w+,\s*mk_tally\s*\*\s*\w+\s*\)",
}


def test_header_declares_and_library_exports_the_tally_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is L.i32
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+listed\s*,\s*unique\s*,\s*best\s*,\s*best_matches\s*;\s*\}\s*mk_tally\s*;", text)
    assert len(L.SIGNATURES["mk_qset_run_tally"][1]) == 6 and L.SIGNATURES["mk_qset_run_tally"][1][3] is ctypes.c_double
    assert len(L.SIGNATURES["mk_query_tally"][1]) == 7 and L.SIGNATURES["mk_query_tally"][1][5] is ctypes.c_double
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert ctypes.sizeof(L.Tally) == 32
    assert [f[0] for f in L.Tally._fields_] == ["listed", "unique", "best", "best_matches"]


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    assert lib.mk_tally_reset(None, None, 4) == -1
    assert lib.mk_qset_run_tally(None, None, 10, 1.0, None, 4) == -1
    assert lib.mk_tally_read(None, None, 4, None) == -1
    assert lib.mk_query_tally(None, None, None, 4, 10, 1.0, None) == -1
    assert b"null argument" in lib.mk_last_error()


def test_python_has_tally():
    from miekki_amd.index import Miekki
    assert callable(Miekki.tally)


def test_profile_file_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "profile_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "profile_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1000
