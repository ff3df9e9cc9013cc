"""mk_index_extend at the C boundary -- declared, exported, bound, an addition to ABI version 5 -- and the one refusal of
`miekki -M` that needs no index file: with -l.  Nothing here touches a GPU."""
import ctypes
import os
import re
import subprocess

from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "miekki_amd", "miekki")
DECL = r"int\s+mk_index_extend\s*\(\s*mk_ctx\s*\*\s*\w+\s*,\s*mk_ctx\s*\*\s*\w+\s*\)\s*;"


def test_extend_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    assert re.search(DECL, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)                  # an addition: nothing existing changed
    assert hasattr(ctypes.CDLL(L.library_path()), "mk_index_extend")
    res, args = L.SIGNATURES["mk_index_extend"]
    assert res is ctypes.c_int32 and args == [ctypes.c_void_p, ctypes.c_void_p]
    lib = L.load_library()
    assert lib.mk_abi_version() == 5
    # null arguments are refused before any device is looked for
    assert lib.mk_index_extend(None, None) == -1
    assert b"null" in lib.mk_last_error()


def test_the_python_class_has_extend():
    from miekki_amd.index import Miekki
    assert callable(getattr(Miekki, "extend", None))


def test_join_is_refused_with_a_list_build(tmp_path):
    """the joined genomes would have no file names: refused with a message, exit status 1, before any device is touched or
    any file is written"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MIEKKI_WORLD", "MIEKKI_RANK")}
    r = subprocess.run([CLI, "-l", "x.lst", "-M", "y.gz", "-d", "never.gz"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=60, env=env)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 1, out
    assert "-M is not supported with -l" in out and "file names" in out
    assert "Using " not in out and os.listdir(tmp_path) == []
    r = subprocess.run([CLI, "-M", "y.gz"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60, env=env)
    assert r.returncode == 1 and b"needs -i" in r.stdout
    assert os.listdir(tmp_path) == []
