"""Representatives without a GPU: the reference model (tests/representatives_ref.py) on the oracle's rows of the family
tests' planted collections -- what the definition implies, and the cases the device pass has to get right -- and
mk_index_representatives at the C boundary: declared, exported, bound, additions only."""
import ctypes
import os
import re

import numpy as np
import pytest

import families_ref as fr
import representatives_ref as rr
from miekki_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Model:
    def __init__(self, G, fp_bits, seed, reverse=False):
        self.c = c = fr.Collection(G, fp_bits, seed)
        self.a = a = fr.Answer(c.par, c.seqs[::-1] if reverse else c.seqs)
        inter = fr.intersections(a.rows, a.ss, a.gs)
        if reverse:
            inter = inter[::-1, ::-1]                                    # (the threshold is defined on the planted ids)
        self.mi = c.threshold_between_chain_links(inter)
        self.lists = a.lists(10, self.mi)
        self.linked = rr.links(self.lists)
        self.rep = rr.greedy(self.linked)
        self.labels = fr.family_labels(self.lists)


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(fp_bits, reverse=False):
        if (fp_bits, reverse) not in made:
            made[fp_bits, reverse] = Model(1101, 8, 310_000, reverse) if fp_bits == 8 else Model(603, 16, 320_000, reverse)
        return made[fp_bits, reverse]
    return get


@pytest.mark.parametrize("fp_bits, n_reps, n_families", [(8, 1092, 1091), (16, 594, 593)])
def test_model_on_the_planted_collections(models, fp_bits, n_reps, n_families):
    m = models(fp_bits)
    c, rep, labels = m.c, m.rep, m.labels
    rr.check_consequences(rep, m.linked)
    np.testing.assert_array_equal(labels[rep], labels)                   # a representative lies in its member's family
    x, y, z = c.chain
    # the chain's far end is linked with the middle only, which is a member: a representative of its own inside the family
    assert list(rep[[x, y, z]]) == [x, x, z] and labels[x] == labels[z]
    assert not m.linked[x, z]
    assert (rep == np.arange(c.G)).sum() == n_reps and len(set(labels)) == n_families
    assert np.bincount(rep).max() == 5
    for cluster in (c.species_a, c.species_b, c.nested):
        assert list(rep[cluster]) == [min(cluster)] * len(cluster)
    n0, n1 = c.nested
    assert m.lists[n1, n0] and not m.lists[n0, n1]                       # listed in one direction only: by the later id


def test_model_at_the_default_thresholds(models):
    """10, 0.5 * 20: the 8-bit collection's chance matches pass -- dense links inside every set, stars are not families"""
    m = models(8)
    lists = m.a.lists(10, 0.5 * m.c.THRESHOLD)
    linked, labels = rr.links(lists), fr.family_labels(lists)
    rep = rr.greedy(linked)
    rr.check_consequences(rep, linked)
    np.testing.assert_array_equal(labels[rep], labels)
    assert (rep == np.arange(m.c.G)).sum() == 6 and len(set(labels)) == 1 and (rep != labels).sum() == 311
    m16 = models(16)
    rep16 = rr.representatives(m16.a)
    assert (rep16 == np.arange(m16.c.G)).sum() == 593


def test_model_on_the_reversed_order(models):
    """the nested pair's one link now points from the smaller id to the larger: only a representative's claim on what IT lists
    above its set (the propagate step) finds it"""
    m = models(8, reverse=True)
    G = m.c.G
    rr.check_consequences(m.rep, m.linked)
    np.testing.assert_array_equal(m.labels[m.rep], m.labels)
    lo, hi = sorted(G - 1 - g for g in m.c.nested)
    assert m.lists[lo, hi] and not m.lists[hi, lo]
    assert hi // 64 != lo // 64 and hi - lo > 64
    assert m.rep[lo] == lo and m.rep[hi] == lo
    a, b, c = (G - 1 - g for g in m.c.chain)                             # the chain from its other end: c < b < a
    assert m.rep[c] == c and m.rep[b] == c and m.rep[a] == a


DECL = r"int\s+mk_index_representatives\s*\(\s*mk_ctx\s*\*\s*\w*,\s*uint32_t\s+\w+,\s*double\s+\w+,\s*uint32_t\s*\*\s*\w+\s*\)"


def test_header_declares_library_exports_python_binds():
    text = open(os.path.join(ROOT, "include", "miekki_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(DECL, text)
    assert re.search(r"#define\s+MK_ABI_VERSION\s+5\b", text)
    assert hasattr(ctypes.CDLL(L.library_path()), "mk_index_representatives")
    res, args = L.SIGNATURES["mk_index_representatives"]
    assert res is L.i32 and len(args) == 4 and args[2] is ctypes.c_double
    from miekki_amd.index import Miekki
    assert callable(Miekki.representatives)


def test_null_context_is_refused_and_the_version_stays():
    lib = L.load_library()
    assert lib.mk_index_representatives(None, 10, 1.0, None) == -1
    assert b"null argument" in lib.mk_last_error()
    assert lib.mk_abi_version() == 5
    assert (ctypes.sizeof(L.Hit), ctypes.sizeof(L.Params), ctypes.sizeof(L.PackedSeq), ctypes.sizeof(L.Stats)) == (24, 32, 56, 128)
