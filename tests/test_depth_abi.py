"""The depth entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library, bound in
miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  And the writer of `miekki -D`'s
file (host/depth.hpp) under AddressSanitizer + UBSan, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {
    "mk_depth_bytes": r"uint64_t\s+mk_depth_bytes\s*\(\s*const\s+mk_ctx\s*\*\s*\w*\s*\)",
    "mk_depth_reset": r"int\s+mk_depth_reset\s*\(\s*mk_ctx\s*\*\s*\w*,\s*uint8_t\s*\*\s*\w+\s*\)",
    "mk_qset_run_depth": r"int\s+mk_qset_run_depth\s*\(\s*mk_ctx\s*\*\s*\w*,\s*mk_qset\s*\*\s*\w+,\s*uint8_t\s*\*\s*\w+\s*\)",
    "mk_depth_profile": r"int\s+mk_depth_profile\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+uint8_t\s*\*\s*\w+,\s*mk_depth\s*\*\s*\w+,"
                        r"\s*uint64_t\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+\s*\)",
    "mk_query_depth": r"int\s+mk_query_depth\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+,"
                      r"\s*uint32_t\s+\w+,\s*mk_depth\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+\s*\)",
}


def test_header_declares_and_library_exports_the_depth_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
        assert L.SIGNATURES[name][0] is (L.u64 if name == "mk_depth_bytes" else L.i32)
    assert [len(L.SIGNATURES[n][1]) for n in CALLS] == [1, 2, 3, 5, 7]
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)
    assert re.search(r"#define\s+MK_DEPTH_MAX\s+255u\b", text)
    assert re.search(r"typedef\s+struct\s*\{\s*uint64_t\s+sum;\s*uint32_t\s+covered;\s*uint32_t\s+median;\s*\}\s*mk_depth;", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert ctypes.sizeof(L.Tally) == 32
    assert ctypes.sizeof(L.Depth) == 16
    assert (L.Depth.sum.offset, L.Depth.covered.offset, L.Depth.median.offset) == (0, 8, 12)


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    assert lib.mk_depth_bytes(None) == 0
    assert lib.mk_depth_reset(None, None) == -1
    assert lib.mk_qset_run_depth(None, None, None) == -1
    assert lib.mk_depth_profile(None, None, None, None, None) == -1
    assert lib.mk_query_depth(None, None, None, 4, None, None, None) == -1
    assert b"null argument" in lib.mk_last_error()


def test_table_bytes_helper():
    assert L.depth_bytes(9, 8) == 131072 and L.depth_bytes(20, 8) == 256 << 20
    assert L.depth_bytes(17, 16) == 8 << 30 and L.depth_bytes(20, 16) == 64 << 30


def test_python_has_depth():
    from miekki_amd.index import Miekki
    assert callable(Miekki.depth)


def test_depth_file_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "depth_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "depth_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1000
