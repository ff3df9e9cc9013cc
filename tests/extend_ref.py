"""The stream of two indexes joined (mk_index_extend, `miekki -M`), made from their two streams with numpy alone: the
yardstick the join's tests hold the code against, itself held against the oracle's joint build in
tests/test_extend_definition.py.  A stream is what dump_disk writes before gzip (Miekki.cpp:649-680): the 39-byte header,
the columns partition by partition, genome_size, the Bloom filter bytes, sketch_size."""
import struct

import numpy as np

HDR = struct.Struct("<6IQBBIB")


def parts(stream):
    """(header fields, columns [P, G * W], genome_size bytes, Bloom bytes, sketch_size bytes) -- views of the stream"""
    a = np.frombuffer(stream, np.uint8) if not isinstance(stream, np.ndarray) else stream
    f = HDR.unpack(a[:39].tobytes())
    k, h, fpb, nbm, G, bl2, bbits = f[:7]
    W, P = fpb // 8, 1 << h
    o = 39
    cols = a[o:o + P * G * W].reshape(P, G * W); o += P * G * W
    gs = a[o:o + 8 * G]; o += 8 * G
    bloom = a[o:o + bbits // 8]; o += bbits // 8
    ss = a[o:o + 4 * G]; o += 4 * G
    assert o == len(a), "not an index stream"
    return f, cols, gs, bloom, ss


def joined_stream(a, b):
    """the stream of a's genomes followed by b's: a's header with the summed size, the columns side by side in every
    partition, the sizes concatenated, and in every Bloom cell a's byte where it is non-zero and b's otherwise (a cell
    keeps its first writer in genome order, Miekki.cpp:121-131)"""
    fa, ca, gsa, bla, ssa = parts(a)
    fb, cb, gsb, blb, ssb = parts(b)
    assert fa[:3] == fb[:3] and fa[5:7] == fb[5:7], "k, h, fingerprint width and Bloom size must agree"
    hdr = np.frombuffer(HDR.pack(*fa[:4], fa[4] + fb[4], *fa[5:]), np.uint8)
    return np.concatenate([hdr, np.concatenate([ca, cb], axis=1).reshape(-1), gsa, gsb, np.where(bla != 0, bla, blb), ssa, ssb])
