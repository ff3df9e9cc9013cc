"""The query-block scan's compare on its own (scan_kernel.hpp: ne_lanes_block, through the probe mk_probe_ne_lanes): for a
matrix word d and a broadcast fingerprint b, 1 in the lowest bit of every byte (half-word) that differs and 0 where they
are equal.  The short forms -- xor, v_lerp_u8, shift, and at one byte; xor, v_pk_min_u16 at two -- must give what the
five-instruction form gives: EVERY (d, b) pair of a byte in each of the four byte positions, every difference of a half-word
in both positions, with the other bytes (the other half) of d ^ b at 0x00, 0x01, 0x7f, 0x80 and 0xff (0x0000 ... 0xffff): a
carry or a borrow between lanes, a shift that drags a neighbour's bit along, would show there.  The expectation is numpy's."""
import numpy as np
import pytest

import miekki_amd
from miekki_amd import lib as L

pytestmark = pytest.mark.gpu


def probe(width, d, b):
    d, b = np.ascontiguousarray(d, np.uint32), np.ascontiguousarray(b, np.uint32)
    flags = np.empty(len(d), np.uint32)
    ix = miekki_amd.Miekki(21, 12, 8 * width, 33, 20)
    try:
        L.check(ix._lib.mk_probe_ne_lanes(ix._h, width, d.ctypes.data, b.ctypes.data, len(d), flags.ctypes.data))
    finally:
        ix.close()
    return flags


def expected(width, d, b):
    x = (d ^ b).astype(np.uint32)
    lanes = x.view(np.uint8 if width == 1 else np.uint16).reshape(len(x), -1)
    return (lanes != 0).astype(lanes.dtype).view(np.uint32).reshape(len(x))


@pytest.mark.parametrize("pos", range(4))
def test_every_pair_of_bytes(pos):
    """All 65,536 (d byte, b byte) pairs in byte `pos`; the other three bytes of d ^ b at each of five values: b has its byte
    in every position (the fingerprint is broadcast), d the byte under test and, elsewhere, b's byte ^ the other value."""
    db, bb = (a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    ds, bs = [], []
    for other in (0x00, 0x01, 0x7f, 0x80, 0xff):
        b = bb * np.uint32(0x01010101)
        rest = (bb ^ np.uint32(other)) * np.uint32(0x01010101)
        mask = np.uint32(0xff << (8 * pos))
        ds.append((rest & ~mask) | (db << np.uint32(8 * pos)))
        bs.append(b)
    d, b = np.concatenate(ds), np.concatenate(bs)
    assert len(d) == 5 * 65536
    np.testing.assert_array_equal(probe(1, d, b), expected(1, d, b))


@pytest.mark.parametrize("pos", range(2))
def test_every_difference_of_a_half_word(pos):
    """All 65,536 values of d ^ b in half-word `pos`, for the fingerprints 0x0000, 0x1234 and 0xffff, the other half's
    difference at each of five values."""
    x = np.arange(65536, dtype=np.uint32)
    ds, bs = [], []
    for fp in (0x0000, 0x1234, 0xffff):
        for other in (0x0000, 0x0001, 0x7fff, 0x8000, 0xffff):
            b = np.full(65536, fp * 0x00010001, np.uint32)
            diff = (x << np.uint32(16 * pos)) | np.uint32(other << (16 * (1 - pos)))
            ds.append(b ^ diff)
            bs.append(b)
    d, b = np.concatenate(ds), np.concatenate(bs)
    np.testing.assert_array_equal(probe(2, d, b), expected(2, d, b))
