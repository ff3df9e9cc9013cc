"""The family entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library,
bound in miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  And the writer of
`miekki -F`'s file (host/families.hpp) under AddressSanitizer + UBSan, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    "mk_link_reset": r"int\s+mk_link_reset\s*\(\s*mk_ctx\s*\*\s*\w*,\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s+\w+\s*\)",
    "mk_qset_run_link": r"int\s+mk_qset_run_link\s*\(\s*mk_ctx\s*\*\s*\w*,\s*mk_qset\s*\*\s*\w+,\s*const\s+uint32_t\s*\*\s*\w+,\s*uint32_t\s+\w+,"
                        r"\s*double\s+\w+,\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s+\w+\s*\)",
    "mk_link_merge": r"int\s+mk_link_merge\s*\(\s*mk_ctx\s*\*\s*\w*,\s*uint32_t\s*\*\s*\w+,\s*const\s+uint32_t\s*\*\s*\w+,\s*uint32_t\s+\w+\s*\)",
    "mk_link_labels": r"int\s+mk_link_labels\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+uint32_t\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s*\*\s*\w+\s*\)",
    "mk_index_families": r"int\s+mk_index_families\s*\(\s*mk_ctx\s*\*\s*\w*,\s*uint32_t\s+\w+,\s*double\s+\w+,\s*uint32_t\s*\*\s*\w+\s*\)",
}


def test_header_declares_and_library_exports_the_family_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is L.i32
    assert len(L.SIGNATURES["mk_qset_run_link"][1]) == 7 and L.SIGNATURES["mk_qset_run_link"][1][4] is ctypes.c_double
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    assert lib.mk_link_reset(None, None, 4) == -1
    assert lib.mk_qset_run_link(None, None, None, 10, 1.0, None, 4) == -1
    assert lib.mk_link_merge(None, None, None, 4) == -1
    assert lib.mk_link_labels(None, None, 4, None) == -1
    assert lib.mk_index_families(None, 10, 1.0, None) == -1
    assert b"null argument" in lib.mk_last_error()


def test_python_has_families():
    from miekki_amd.index import Miekki
    assert callable(Miekki.families)


def test_family_file_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "families_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-o", exe, os.path.join(ROOT, "tests", "helpers", "families_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1000
