"""The panel entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library, bound in
miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  And the writer of `miekki -S ... -c`'s
file (host/panel.hpp) under AddressSanitizer + UBSan, as a stand-alone program."""
import ctypes
import os
import re
import subprocess

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX, PANEL, CPANEL = r"mk_ctx\s*\*\s*\w*", r"uint8_t\s*\*\s*\w+", r"const\s+uint8_t\s*\*\s*\w+"
CALLS = {
    "mk_panel_bytes": r"uint64_t\s+mk_panel_bytes\s*\(\s*const\s+" + CTX + r"\s*\)",
    "mk_panel_reset": r"int\s+mk_panel_reset\s*\(\s*" + CTX + r",\s*" + PANEL + r"\s*\)",
    "mk_qset_run_panel": r"int\s+mk_qset_run_panel\s*\(\s*" + CTX + r",\s*mk_qset\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*" + PANEL + r"\s*\)",
    "mk_panel_count": r"int\s+mk_panel_count\s*\(\s*" + CTX + r",\s*" + CPANEL + r",\s*uint32_t\s+\w+,\s*uint32_t\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+\s*\)",
    "mk_panel_slot": r"int\s+mk_panel_slot\s*\(\s*" + CTX + r",\s*" + CPANEL + r",\s*uint32_t\s+\w+,\s*uint32_t\s*\*\s*\w+\s*\)",
    "mk_query_panel": r"int\s+mk_query_panel\s*\(\s*" + CTX + r",\s*const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+,"
                      r"\s*const\s+uint64_t\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s*\*\s*\w+,\s*uint64_t\s*\*\s*\w+\s*\)",
}


def test_header_declares_and_library_exports_the_panel_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
        assert L.SIGNATURES[name][0] is (L.u64 if name == "mk_panel_bytes" else L.i32)
    assert [len(L.SIGNATURES[n][1]) for n in CALLS] == [1, 2, 4, 5, 4, 7]
    assert L.SIGNATURES["mk_qset_run_panel"][1][2] is L.u32 and L.SIGNATURES["mk_panel_count"][1][2] is L.u32
    assert L.SIGNATURES["mk_panel_slot"][1][2] is L.u32 and L.SIGNATURES["mk_query_panel"][1][4] is L.u32
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)
    assert re.search(r"#define\s+MK_PANEL_SLOTS\s+8u\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert (ctypes.sizeof(L.Tally), ctypes.sizeof(L.CladeTally), ctypes.sizeof(L.Depth), ctypes.sizeof(L.Pick)) == (32, 40, 16, 24)
    assert (L.Depth.sum.offset, L.Depth.covered.offset, L.Depth.median.offset) == (0, 8, 12)


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    assert lib.mk_panel_bytes(None) == 0
    assert lib.mk_panel_reset(None, None) == -1
    assert lib.mk_qset_run_panel(None, None, 0, None) == -1
    assert lib.mk_panel_count(None, None, 8, None, None) == -1
    assert lib.mk_panel_slot(None, None, 0, None) == -1
    assert lib.mk_query_panel(None, None, None, None, 4, None, None) == -1
    assert b"null argument" in lib.mk_last_error()


def test_table_bytes_helper():
    assert L.panel_bytes(9, 8) == 131072 and L.panel_bytes(20, 8) == 256 << 20
    assert L.panel_bytes(17, 16) == 8 << 30 and L.panel_bytes(20, 16) == 64 << 30
    assert L.panel_bytes(14, 8) == L.depth_bytes(14, 8) == 8 * L.cover_bytes(14, 8)


def test_python_has_panel():
    from miekki_amd.index import Miekki
    assert callable(Miekki.panel)


def test_panel_file_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "panel_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "panel_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1000
