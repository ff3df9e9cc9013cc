"""The cover entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library, bound in
miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  And the writer of `miekki -C`'s
file (host/cover.hpp) under AddressSanitizer + UBSan, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    "mk_cover_bytes": r"uint64_t\s+mk_cover_bytes\s*\(\s*const\s+mk_ctx\s*\*\s*\w*\s*\)",
    "mk_cover_reset": r"int\s+mk_cover_reset\s*\(\s*mk_ctx\s*\*\s*\w*,\s*uint32_t\s*\*\s*\w+\s*\)",
    "mk_qset_run_cover": r"int\s+mk_qset_run_cover\s*\(\s*mk_ctx\s*\*\s*\w*,\s*mk_qset\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+\s*\)",
    "mk_cover_count": r"int\s+mk_cover_count\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+uint32_t\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+\s*\)",
    "mk_query_cover": r"int\s+mk_query_cover\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+,"
                      r"\s*uint32_t\s+\w+,\s*uint32_t\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+\s*\)",
}


def test_header_declares_and_library_exports_the_cover_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
        assert L.SIGNATURES[name][0] is (L.u64 if name == "mk_cover_bytes" else L.i32)
    assert [len(L.SIGNATURES[n][1]) for n in CALLS] == [1, 2, 3, 4, 6]
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert ctypes.sizeof(L.Tally) == 32


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    assert lib.mk_cover_bytes(None) == 0
    assert lib.mk_cover_reset(None, None) == -1
    assert lib.mk_qset_run_cover(None, None, None) == -1
    assert lib.mk_cover_count(None, None, None, None) == -1
    assert lib.mk_query_cover(None, None, None, 4, None, None) == -1
    assert b"null argument" in lib.mk_last_error()


def test_table_bytes_helper():
    assert L.cover_bytes(9, 8) == 16384 and L.cover_bytes(20, 8) == 32 << 20 and L.cover_bytes(20, 16) == 8 << 30


def test_python_has_cover():
    from miekki_amd.index import Miekki
    assert callable(Miekki.cover)


def test_cover_file_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "cover_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "cover_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1000
