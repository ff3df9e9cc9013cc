"""The winners entry points at the C boundary, without a GPU: declared in include/miekki_hip.h, exported by the library, bound in
miekki_amd.lib -- additions only: the ABI version and the struct layouts stay where they were.  And the order
(miekki_amd/csrc/cover_order.hpp) and the writer of `miekki -W`'s file (host/winners.hpp) under AddressSanitizer + UBSan, as a
stand-alone program whose output is compared with tests/winners_ref.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import winners_ref as wr
from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32P, U64P = r"uint32_t\s*\*\s*\w+", r"uint64_t\s*\*\s*\w+"
CALLS = {
    "mk_cover_assign": rf"int\s+mk_cover_assign\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+{U32P},\s*const\s+{U32P},\s*{U32P},\s*{U64P}\s*\)",
    "mk_cover_winners": rf"int\s+mk_cover_winners\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+{U32P},\s*{U32P},\s*{U32P},\s*{U64P},\s*{U64P}\s*\)",
    "mk_query_cover_winners": r"int\s+mk_query_cover_winners\s*\(\s*mk_ctx\s*\*\s*\w*,\s*const\s+char\s*\*\s*const\s*\*\s*\w+,\s*const\s+uint64_t\s*\*\s*\w+,"
                              rf"\s*uint32_t\s+\w+,\s*{U32P},\s*{U32P},\s*{U64P},\s*{U64P}\s*\)",
}


def test_header_declares_and_library_exports_the_winners_calls():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(L.library_path())
    for name, decl in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is L.i32
    assert [len(L.SIGNATURES[n][1]) for n in CALLS] == [5, 6, 8]
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
    assert ctypes.sizeof(L.Tally) == 32


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    assert lib.mk_cover_assign(None, None, None, None, None) == -1
    assert lib.mk_cover_winners(None, None, None, None, None, None) == -1
    assert lib.mk_query_cover_winners(None, None, None, 4, None, None, None, None) == -1
    assert b"null argument" in lib.mk_last_error()


def test_python_has_cover_winners():
    from miekki_amd.index import Miekki
    assert callable(Miekki.cover_winners) and callable(Miekki.cover)


def test_order_and_file_writer_under_sanitizers(tmp_path):
    exe = str(tmp_path / "winners_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "miekki_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "winners_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), r.stdout[-2000:] + r.stderr[-2000:]
    cases = r.stdout.split("case ")[1:]
    names = [c.split("\n", 1)[0] for c in cases]
    for want in ("equal_shares_different_covered", "empty_sketches", "products_near_2_56", "all_equal"):
        assert want in names
    assert len(cases) >= 40
    for c in cases:
        name, rest = c.split("\n", 1)
        head, tail = rest.split("file\n", 1)
        rows = {l.split(" ", 1)[0]: np.array(l.split()[1:], np.uint64) for l in head.splitlines()}
        cov, ss = rows["cov"], rows["ss"]
        want = wr.order(cov, ss)
        assert rows["order"].tolist() == want.tolist(), name
        assert rows["rank"].tolist() == wr.rank_of(want).tolist(), name
        body, after = tail.split("end ", 1)
        won = rows["won"]
        assert body.encode() == wr.format_winners(won, cov, ss), name
        lines = after.splitlines()
        assert int(lines[0]) == int((won > 0).sum())
        claimed = int(sum(int(x) for x in won))
        assert lines[1].encode() == wr.summary_line(3 * len(cov), claimed, claimed + 7, won), name
    all_equal = cases[names.index("all_equal")]
    assert "order " + " ".join(str(i) for i in range(70)) + "\n" in all_equal
