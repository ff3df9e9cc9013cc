"""The one chunk pass of the query path (api_query.hip: for_chunks) cut into several chunks: mk_qset_run, mk_query,
mk_qset_run_list and mk_qset_run_link + mk_link_labels must return, bit for bit, what they return in one chunk.

A set takes more than one chunk only at full size, so MIEKKI_CHUNK_QUERIES caps a chunk's queries: 16 is a multiple of the
query groups' sixteen -- every chunk starts on a group boundary -- and 24 is not: the second chunk starts inside a group.
MIEKKI_SLAB_MIN_QUERIES=0 and MIEKKI_SLAB_MIB=4 (four partition ranges at -h 14) give the 40 short queries the range table
and the query groups.  The plain schedule's set is made of long reads alone: one long read among short queries makes a mixed
set, whose plain part is that one read -- that set is run as well, for the shell over two parts.  One fresh process per
setting (tests/chunk_pass_worker.py), all three at once."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CAPS = [None, 16, 24]
RESULTS = ["run_count", "run_cand", "query_n", "query_hits", "query_act", "list_off", "list_hits", "labels"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunk_pass")
    procs = {}
    for cap in CAPS:
        env = dict(os.environ, MIEKKI_SLAB_MIN_QUERIES="0", MIEKKI_SLAB_MIB="4")
        env.pop("MIEKKI_CHUNK_QUERIES", None)
        if cap:
            env["MIEKKI_CHUNK_QUERIES"] = str(cap)
        procs[cap] = subprocess.Popen([sys.executable, os.path.join(HERE, "chunk_pass_worker.py"), str(d / f"cap_{cap}.npz")],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for cap, p in procs.items():
        text = p.communicate(timeout=300)[0]
        assert p.returncode == 0, text.decode(errors="replace")[-3000:]
        out[cap] = dict(np.load(d / f"cap_{cap}.npz"))
    return out


def test_the_sets_take_the_schedules_and_the_chunks_they_are_meant_to(runs):
    """scan launches of the four passes over a set, (all, of the slab schedule): 40 and 36 queries are 3 chunks of at most
    16 and 2 of at most 24"""
    base = {name: int(runs[None][f"{name}_launches"][0]) for name in ("long", "mixed")}
    for cap, chunks in ((None, 1), (16, 3), (24, 2)):
        allk, slab = (int(x) for x in runs[cap]["short_launches"])
        assert allk == slab == 4 * chunks                        # 40 short queries: the slab schedule alone, once per chunk
        allk, slab = (int(x) for x in runs[cap]["long_launches"])
        assert slab == 0 and allk == chunks * base["long"] > 0   # 36 long reads: the plain schedule alone
        allk, slab = (int(x) for x in runs[cap]["mixed_launches"])
        assert slab == 4 * chunks and allk - slab == base["mixed"] - 4 > 0    # a slab part of 40 and a plain part of one
    one = runs[None]
    assert one["short_run_count"].min() >= 10 and one["long_run_count"].min() >= 10    # every query finds its species
    assert len(one["short_list_hits"]) >= 40 * 16 and len(set(one["short_labels"][:48])) == 3


@pytest.mark.parametrize("cap", CAPS[1:])
@pytest.mark.parametrize("name", ["short", "long", "mixed"])
def test_chunked_passes_return_the_bytes_of_one_chunk(runs, name, cap):
    for r in RESULTS:
        one, cut = runs[None][f"{name}_{r}"], runs[cap][f"{name}_{r}"]
        assert one.dtype == cut.dtype and one.shape == cut.shape and one.tobytes() == cut.tobytes(), r
