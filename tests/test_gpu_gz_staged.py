"""The inflater's batches in steps (mk_gz_open / mk_gz_stage / mk_gz_put / mk_gz_put_span / mk_gz_run) and the memory a context
keeps for them between batches: device blocks taken again, outgrown and trimmed, page-locked pieces lent and taken back,
several threads putting side by side.  Lengths and statuses are held against zlib and the FASTA rule (header lines and line
feeds do not count), indexes against the oracle's, byte for byte."""
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

K, H = 21, 10
OK, NOT_GZIP = 0, 2
ERR_ARG = -1
PIECES = 24                                                           # pieces a context lends at most (16 MiB each)


def gz(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def gunzip_members(blob):
    """every member's text, as zstr reads a file; None: not (only) gzip members"""
    out = b""
    while blob:
        d = zlib.decompressobj(47)
        try:
            out += d.decompress(blob)
        except zlib.error:
            return None
        if not d.eof:
            return None
        blob = d.unused_data
    return out


class File:
    """a genome file: its bytes, and what zlib and the FASTA rule say of it"""
    def __init__(self, blob):
        self.blob = blob
        text = gunzip_members(blob) if blob[:2] == b"\x1f\x8b" else None
        self.status = OK if text is not None else NOT_GZIP
        self.seq = b"".join(l for l in (text or b"").split(b"\n") if not l.startswith(b">"))
        self.len = len(self.seq)


def genome_text(i):
    n = 2000 + (i * 7919) % 28001                                     # 2 to 30 kB
    return synth.fasta("g%d" % i, synth.genome_bases(5000 + i, 0, n), 70)


@pytest.fixture(scope="module")
def files():
    """sixty-four gzip'd genomes, levels 1, 6 and 9 in turn"""
    return [File(gz(genome_text(i), (1, 6, 9)[i % 3])) for i in range(64)]


def new_index():
    import miekki_amd
    return miekki_amd.Miekki(K, H, 8, 32, 10)


def oracle_bytes(fs):
    from oracle import oracle as orc
    o = orc.OracleMiekki(K, H, 8, 32, 10)
    o.insert_sequences([f.seq for f in fs if f.status == OK and f.len >= K])
    raw = bytearray(o.serialize().tobytes()); raw[32] = 0; raw[38] = 0
    return raw


def index_bytes(ix):
    raw = bytearray(b"".join(ix.serialize())); raw[32] = 0; raw[38] = 0
    return raw


class Batch:
    """mk_gz_open ... mk_gz_free over a list of Files"""
    def __init__(self, ix, fs):
        self.ix, self.lib, self.fs, self.n = ix, ix._lib, fs, len(fs)
        self.h = C.c_void_p()
        sizes = (C.c_uint64 * self.n)(*[len(f.blob) for f in fs])
        assert self.lib.mk_gz_open(ix._h, sizes, self.n, C.byref(self.h)) == 0
        self.cap = 0

    def stage(self):
        cap = C.c_uint64()
        p = self.lib.mk_gz_stage(self.h, C.byref(cap))
        if p:
            self.cap = cap.value
        return p

    def put(self, i, at, data, nbytes, staged):
        return self.lib.mk_gz_put(self.h, i, at, data, nbytes, staged)

    def put_loose(self, idx=None):
        for i in (range(self.n) if idx is None else idx):
            assert self.put(i, 0, self.fs[i].blob, len(self.fs[i].blob), 0) == 0

    def put_staged(self, idx=None, split=None):
        """a piece per file; file `split` in two pieces, the second at at > 0"""
        for i in (range(self.n) if idx is None else idx):
            blob = self.fs[i].blob
            cuts = [0, len(blob)] if i != split else [0, len(blob) // 2, len(blob)]
            for lo, hi in zip(cuts, cuts[1:]):
                p = self.stage()
                assert p and hi - lo <= self.cap
                C.memmove(p, blob[lo:hi], hi - lo)
                assert self.put(i, lo, p, hi - lo, 1) == 0

    def layout(self):
        off = (C.c_uint64 * (self.n + 1))()
        assert self.lib.mk_gz_layout(self.h, off) == 0
        return list(off)

    def put_span(self, first, count, off):
        """files first .. first + count as the batch's input holds them: each at its place, zeros up to the next"""
        p = self.stage()
        total = off[first + count] - off[first]
        assert p and total <= self.cap
        C.memset(p, 0, total)
        for i in range(first, first + count):
            C.memmove(p + off[i] - off[first], self.fs[i].blob, len(self.fs[i].blob))
        assert self.lib.mk_gz_put_span(self.h, first, count, p, total, 1) == 0

    def put_spans(self, run):
        off = self.layout()
        for first in range(0, self.n, run):
            self.put_span(first, min(run, self.n - first), off)

    def run(self):
        assert self.lib.mk_gz_run(self.h) == 0

    def results(self):
        status, lens = [], []
        for i in range(self.n):
            ln, st = C.c_uint64(), C.c_int32()
            assert self.lib.mk_gz_sequence(self.h, i, C.byref(ln), C.byref(st)) == 0
            status.append(st.value); lens.append(ln.value)
        return status, lens

    def check(self):
        status, lens = self.results()
        print("statuses", status, "lengths", lens)
        assert status == [f.status for f in self.fs]
        assert lens == [f.len for f in self.fs]
        return status, lens

    def append(self):
        which = [i for i, f in enumerate(self.fs) if f.status == OK and f.len >= K]
        for g0 in range(0, len(which), 64):
            part = which[g0:g0 + 64]
            assert self.lib.mk_index_append_gz(self.ix._h, self.h, (C.c_uint32 * len(part))(*part), len(part)) == 0

    def free(self):
        self.lib.mk_gz_free(self.h)
        self.h = None


def test_three_ways_in_one_result(files):
    a = genome_text(100)
    twelve = files[:9] + [File(gz(b"")), File(gz(a[:len(a) // 2], 6) + gz(a[len(a) // 2:], 1)), File(genome_text(101))]
    assert [f.status for f in twelve] == [OK] * 11 + [NOT_GZIP] and twelve[9].len == 0 and twelve[10].len == 100 * 7919 % 28001 + 2000
    want = oracle_bytes(twelve)
    seen = []
    for route in ("loose", "staged", "spans"):
        ix = new_index()
        try:
            b = Batch(ix, twelve)
            if route == "loose":
                b.put_loose()
            elif route == "staged":
                b.put_staged(split=4)
            else:
                b.put_spans(4)
            b.run()
            seen.append(b.check())
            b.append()
            assert ix._lib.mk_sync(ix._h) == 0
            b.free()
            assert index_bytes(ix) == want, route
        finally:
            ix.close()
    assert seen[0] == seen[1] == seen[2]


def test_blocks_kept_outgrown_trimmed(files):
    ix = new_index()
    order = []
    try:
        def whole(fs):
            b = Batch(ix, fs)
            b.put_staged()
            b.run(); b.check(); b.append(); b.free()
            order.extend(fs)
        whole(files[0:8]); whole(files[8:10]); whole(files[10:26])      # kept blocks fit, are too large, are outgrown
        ix._lib.mk_gz_trim(ix._h)
        whole(files[26:34])
        A, B = Batch(ix, files[34:38]), Batch(ix, files[38:42])          # two batches open at once
        A.put_staged(); B.put_spans(4)
        B.run(); B.check(); B.append(); order.extend(B.fs)
        A.run(); A.check(); A.append(); order.extend(A.fs)
        A.free(); B.free()
        assert ix._lib.mk_sync(ix._h) == 0
        assert index_bytes(ix) == oracle_bytes(order)
    finally:
        ix.close()
    for rep in range(3):                                              # destroyed right behind mk_gz_free: the next blocks may be in the making
        ix = new_index()
        b = Batch(ix, files[rep * 4:rep * 4 + 4])
        b.put_loose(); b.run(); b.check(); b.append(); b.free()
        ix.close()


def test_the_piece_pool_s_edges(files):
    ix = new_index()
    try:
        b = Batch(ix, files[:2])
        held = [b.stage() for _ in range(PIECES)]
        assert all(held) and len(set(held)) == PIECES and b.cap == 16 << 20
        assert b.stage() is None                                      # every piece is in the caller's hands
        assert b.put(0, 0, held.pop(), 0, 1) == 0                     # nothing to copy: the piece is the pool's again
        held.append(b.stage())
        assert held[-1] and b.stage() is None
        stranger = np.zeros(4096, np.uint8)
        assert b.put(0, 0, stranger.ctypes.data, 16, 1) == ERR_ARG    # staged, but no piece
        assert b.put(0, 0, held.pop(), len(files[0].blob) + 1, 1) == ERR_ARG     # beyond the file's size: refused, the piece taken back
        held.append(b.stage())
        assert held[-1] and len(set(held)) == PIECES and b.stage() is None
        while held:
            assert b.put(1, 0, held.pop(), 0, 1) == 0
        b.run()
        assert b.results()[0] == [NOT_GZIP, NOT_GZIP]                 # (a file never put reads as empty)
        assert b.put(0, 0, files[0].blob, len(files[0].blob), 0) == ERR_ARG      # the batch has run
        b.free()
    finally:
        ix.close()


def test_many_hands(files):
    want = oracle_bytes(files)
    seen = []
    for hands in (1, 4):
        ix = new_index()
        try:
            b = Batch(ix, files)
            off = b.layout()
            failed = []
            def work(t):
                try:
                    for first in range(8 * t, 64, 8 * hands):
                        b.put_span(first, 8, off)
                except BaseException as e:                             # (an assertion on a thread of its own is lost otherwise)
                    failed.append(e)
            threads = [threading.Thread(target=work, args=(t,)) for t in range(hands)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not failed, failed
            b.run()
            seen.append(b.check())
            b.append()
            assert ix._lib.mk_sync(ix._h) == 0
            b.free()
            assert index_bytes(ix) == want, hands
        finally:
            ix.close()
    assert seen[0] == seen[1]
