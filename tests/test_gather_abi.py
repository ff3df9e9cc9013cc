"""The gather entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library, bound in
miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  And the writer of `miekki -G`'s
file (host/gather.hpp) under AddressSanitizer + UBSan, as a stand-alone program, against tests/gather_ref.py's formats."""
import ctypes
import os
import re
import subprocess

import numpy as np

import gather_ref as gr
from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P, U64P = r"uint32_t\s*\*\s*\w+", r"uint64_t\s*\*\s*\w+"
TAIL = r"\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*mk_pick\s*\*\s*\w+,\s*" + U32P + r",\s*" + U64P + r",\s*" + U64P + r"\s*\)"
CALLS = {
    "mk_cover_gather": r"int\s+mk_cover_gather\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+uint32_t\s*\*\s*\w+,\s*const\s+uint8_t\s*\*\s*\w+," + TAIL,
    "mk_query_cover_gather": r"int\s+mk_query_cover_gather\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+,"
                             r"\s*uint32_t\s+\w+,\s*int\s+\w+," + TAIL,
}


def test_header_declares_and_library_exports_the_gather_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is L.i32
    assert [len(L.SIGNATURES[n][1]) for n in CALLS] == [9, 11]
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+genome,\s*fresh,\s*covered,\s*sketch_size;\s*uint64_t\s+depth_sum;\s*\}\s*mk_pick;", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert (ctypes.sizeof(L.Tally), ctypes.sizeof(L.Depth)) == (32, 16)
    assert ctypes.sizeof(L.Pick) == 24
    assert [getattr(L.Pick, f).offset for f in ("genome", "fresh", "covered", "sketch_size", "depth_sum")] == [0, 4, 8, 12, 16]
    from miekki_amd.index import Miekki
    assert Miekki.PICK_DTYPE == gr.PICK and gr.PICK.itemsize == 24


def test_null_arguments_and_min_new_zero_are_refused_without_a_device():
    lib = L.load_library()
    picks = (L.Pick * 4)()
    n, cells, explained = ctypes.c_uint32(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    out = (picks, ctypes.byref(n), ctypes.byref(cells), ctypes.byref(explained))
    fake = ctypes.c_void_p(64)                                             # never looked at: the refusals come first
    assert lib.mk_cover_gather(None, fake, None, 1, 0, *out) == -1
    assert b"null argument" in lib.mk_last_error()
    assert lib.mk_cover_gather(None, None, None, 1, 0, *out) == -1
    assert lib.mk_cover_gather(None, fake, None, 0, 0, *out) == -1
    assert lib.mk_query_cover_gather(None, None, None, 4, 0, 1, 0, *out) == -1
    assert lib.mk_query_cover_gather(None, None, None, 0, 1, 0, 0, *out) == -1
    assert (n.value, cells.value, explained.value) == (7, 7, 7) and not bytes(picks).strip(b"\0")


def test_python_has_gather():
    from miekki_amd.index import Miekki
    assert callable(Miekki.gather)


def test_gather_file_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gather_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "gather_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 1000
    # one fixed input, without and with the depth field, against the yardstick's formats
    r = subprocess.run([exe, "show"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    picks = np.zeros(3, gr.PICK)
    picks[0], picks[1], picks[2] = (7, 30, 41, 500, 95), (1003, 30, 30, 480, 1 << 40), (0, 1, 4294967295, 4294967295, 0)
    line = gr.summary_line(620, 61, 99, 3, 10) + b"\n"
    assert r.stdout == gr.format_gather(picks) + line + gr.format_gather(picks, True) + line
