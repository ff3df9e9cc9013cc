"""mk_qset_upload_reads at the C boundary, without a GPU: declared in include/miekki_hip.h as the issue states it, exported by
the library, bound in miekki_amd.lib -- an addition: the ABI version and the struct layouts stay where they were."""
import ctypes
import os
import re

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PP, _U64 = r"\s*const\s+char\s*\*\s*const\s*\*\s*\w+,", r"\s*const\s+uint64_t\s*\*\s*\w+,"
DECL = (r"int\s+mk_qset_upload_reads\s*\(\s*mk_ctx\s*\*\s*\w*," + _PP + _U64 + _PP + _PP + _U64 + _PP +
        r"\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*mk_qset\s*\*\s*\*\s*\w+\s*\)")


def test_header_declares_and_library_exports_the_call():
    raw = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(DECL, text), "mk_qset_upload_reads is not declared as the issue states it"
    assert hasattr(ctypes.CDLL(L.library_path()), "mk_qset_upload_reads")
    res, args = L.SIGNATURES["mk_qset_upload_reads"]
    assert res is L.i32 and len(args) == 10 and args[7] is L.u32 and args[8] is L.u32
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)
    # the comment above the declaration states the definition and cites the reference's lines
    comment = raw[:raw.index("int mk_qset_upload_reads")].rsplit("/*", 1)[1]
    for word in ("Miekki.cpp:150-197", "214-224", "135-146", "phred + 33", "33 + min_qual", "maximal runs", "strict", "junction",
                 "MK_ERR_UNSUPPORTED", "MK_ERR_ARG", "4,096"):
        assert word in comment, word


def test_version_and_layouts_are_unmoved():
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)


def test_null_arguments_are_refused_without_a_device():
    lib = L.load_library()
    qs = ctypes.c_void_p()
    assert lib.mk_qset_upload_reads(None, None, None, None, None, None, None, 4, 20, ctypes.byref(qs)) == -1
    assert b"null argument" in lib.mk_last_error()


def test_python_has_the_three_calls():
    from miekki_amd.index import Miekki
    for name in ("read_set", "read_scores", "query_reads"):
        assert callable(getattr(Miekki, name))
