"""The hierarchy entry points at the C boundary, without a GPU: declared in include/miekki_hip.h as the issue states them,
exported by the library, bound in miekki_amd.lib -- additions only: the ABI version stays where it was."""
import ctypes
import os
import re

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX, U32, U32P = r"mk_ctx\s*\*\s*\w+", r"uint32_t\s+\w+", r"uint32_t\s*\*\s*\w+"
LEVELS = r"const\s+mk_level\s*\*\s*\w+"
CALLS = {
    "mk_qset_run_link_levels": (7, r"int\s+mk_qset_run_link_levels\s*\(\s*" + CTX + r",\s*mk_qset\s*\*\s*\w+,\s*const\s+" + U32P + r",\s*" + LEVELS +
                                r",\s*" + U32 + r",\s*" + U32P + r"\s*,\s*" + U32 + r"\s*\)"),
    "mk_link_fold_levels": (4, r"int\s+mk_link_fold_levels\s*\(\s*" + CTX + r",\s*" + U32P + r",\s*" + U32 + r",\s*" + U32 + r"\s*\)"),
    "mk_index_hierarchy": (4, r"int\s+mk_index_hierarchy\s*\(\s*" + CTX + r",\s*" + LEVELS + r",\s*" + U32 + r",\s*" + U32P + r"\s*\)"),
}


def header():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_and_library_exports_the_hierarchy_calls():
    text = header()
    lib = ctypes.CDLL(L.library_path())
    for name, (n_args, decl) in CALLS.items():
        assert re.search(decl, text), f"{name} is not declared as the issue states it"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES and L.SIGNATURES[name][0] is L.i32
        assert len(L.SIGNATURES[name][1]) == n_args
    assert re.search(r"#define\s+MK_MAX_LEVELS\s+8\b", text) and L.MAX_LEVELS == 8
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+min_score;\s*uint32_t\s+reserved;\s*double\s+min_intersection;\s*\}\s*mk_level;", text)
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)


def test_level_layout_and_version():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert ctypes.sizeof(L.Level) == 16
    assert [getattr(L.Level, f).offset for f in ("min_score", "reserved", "min_intersection")] == [0, 4, 8]
    assert L.SIGNATURES["mk_qset_run_link_levels"][1][3] is L.SIGNATURES["mk_index_hierarchy"][1][1]
    assert L.SIGNATURES["mk_index_hierarchy"][1][1]._type_ is L.Level


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    lv = (L.Level * 2)(L.Level(10, 0, 10.0), L.Level(20, 0, 20.0))
    fake = ctypes.c_void_p(64)                                             # never looked at: the refusals come first
    out = (ctypes.c_uint32 * 8)(*([7] * 8))
    assert lib.mk_qset_run_link_levels(None, fake, fake, lv, 2, fake, 4) == -1
    assert b"null argument" in lib.mk_last_error()
    assert lib.mk_qset_run_link_levels(None, None, None, None, 2, None, 4) == -1
    assert lib.mk_link_fold_levels(None, fake, 4, 2) == -1
    assert b"null argument" in lib.mk_last_error()
    assert lib.mk_index_hierarchy(None, lv, 2, out) == -1
    assert b"null argument" in lib.mk_last_error()
    assert list(out) == [7] * 8


def test_python_has_hierarchy():
    from miekki_amd.index import Miekki
    assert callable(Miekki.hierarchy)
