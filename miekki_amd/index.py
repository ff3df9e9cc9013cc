"""Python mirror of the reference's `Miekki` class for the hot path (Miekki.h:34-137).

Same member names, argument meaning and error behaviour as the reference so that
parity tests read like calls into it.  Every computation goes through the C ABI
of libmiekki_hip.so; when the library or the GPU is missing, construction raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import gzip
import os
import struct
from collections import namedtuple

import numpy as np

from . import lib as L

# Miekki.h:27-31
SimilarityScore = namedtuple("SimilarityScore", "genome matches jaccard intersection")

_HDR = struct.Struct("<6IQBBIB")     # 39 bytes, unpadded
assert _HDR.size == 39
_HIT_DTYPE = np.dtype([("genome", "<u4"), ("matches", "<u4"), ("jaccard", "<f8"), ("intersection", "<f8")])   # mk_hit
assert _HIT_DTYPE.itemsize == C.sizeof(L.Hit)


def _node_arrays(nodes):
    """(lo, hi) as uint32 arrays of a taxonomy given as a sequence of (lo, hi) (Miekki.lca, Miekki.taxon_cover)"""
    pairs = []
    for node in nodes:
        lo, hi = node
        for v in (lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 32:
                raise ValueError("a node is a pair (lo, hi) of genome ids, integers below 2^32")
        pairs.append((int(lo), int(hi)))
    return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.uint32)


class Miekki:
    def __init__(self, kmer_size=31, number_minimizer_log2=17, number_bit_minimizer=8,
                 bloom_size_log2=33, threshold=200, device=0, genome_id_base=0):
        self._lib = L.load_library()
        self._p = L.Params(kmer_size, number_minimizer_log2, number_bit_minimizer, bloom_size_log2,
                           int(threshold), device, genome_id_base, 0)
        h = C.c_void_p()
        st = self._lib.mk_create(C.byref(self._p), C.byref(h))
        if st == -2:
            raise NotImplementedError("not implemented")          # Miekki.cpp:235-237
        L.check(st)
        self._h = h
        self.file_names = []                                       # Miekki.h:59 (never persisted)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mk_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- members of the reference object
    kmer_size = property(lambda s: s._p.k)
    number_minimizer_log2 = property(lambda s: s._p.h)
    number_minimizer = property(lambda s: 1 << s._p.h)
    number_bit_minimizer = property(lambda s: s._p.fp_bits)
    bloom_size_log2 = property(lambda s: s._p.bloom_log2)
    bloom_size = property(lambda s: (1 << s._p.bloom_log2) if s._p.bloom_log2 else 0)
    threshold = property(lambda s: s._p.threshold)
    index_size = property(lambda s: s._lib.mk_index_size(s._h))
    W = property(lambda s: s._p.fp_bits // 8)

    @property
    def genome_size(self):
        out = np.zeros(self.index_size, np.uint64)
        L.check(self._lib.mk_index_export_sizes(self._h, out.ctypes.data, None))
        return out

    @property
    def sketch_size(self):
        out = np.zeros(self.index_size, np.uint32)
        L.check(self._lib.mk_index_export_sizes(self._h, None, out.ctypes.data))
        return out

    def reserve(self, n_genomes):
        L.check(self._lib.mk_reserve(self._h, n_genomes))

    def compress_index(self):
        """Miekki::compress_index (Miekki.cpp:863-868) for the rows beyond the matrix's HBM budget: returns
        (raw bytes, packed bytes) of those rows -- equal when nothing was packed (no cold rows, or nothing to gain)."""
        raw, packed = C.c_uint64(0), C.c_uint64(0)
        L.check(self._lib.mk_index_compress(self._h, C.byref(raw), C.byref(packed)))
        return raw.value, packed.value

    def decompress_index(self):
        """Miekki::decompress_index (Miekki.cpp:872-877)."""
        L.check(self._lib.mk_index_decompress(self._h))

    def insert_synthetic_strains(self, first_id, n, length, strains, rate_ppm):
        L.check(self._lib.mk_index_append_synthetic_strains(self._h, first_id, n, length, strains, rate_ppm))
        self.file_names += [f"strain:{first_id + i}" for i in range(n)]

    def select(self, ids):
        """Keep the genomes `ids` (as the index reports them, distinct), in that order, in place (mk_index_select):
        genome j of the index becomes the genome that was ids[j].  The Bloom filter stays as it is; file_names follow
        when they are known.  A refused list (empty, an unknown or repeated id) leaves the index as it was."""
        ids = np.ascontiguousarray(ids, np.uint32)
        named = len(self.file_names) == self.index_size
        L.check(self._lib.mk_index_select(self._h, ids.ctypes.data, len(ids)))
        if named:
            base = self._p.genome_id_base
            self.file_names = [self.file_names[int(g) - base] for g in ids]

    def extend(self, other):
        """Append the genomes of `other`, a Miekki on the same device with the same k, h, fingerprint width and Bloom
        size, behind this index's, in their order (mk_index_extend): the index of a build of this index's genomes
        followed by other's, bit for bit.  `other` stays open and unchanged.  file_names are concatenated when both
        lists are complete, and emptied otherwise.  A refused call leaves the index as it was."""
        if not isinstance(other, Miekki) or not getattr(other, "_h", None):
            raise TypeError("extend takes an open Miekki")
        named = len(self.file_names) == self.index_size and len(other.file_names) == other.index_size
        L.check(self._lib.mk_index_extend(self._h, other._h))
        self.file_names = self.file_names + list(other.file_names) if named else []

    def stats(self):
        s = L.Stats()
        L.check(self._lib.mk_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.Stats._fields_}

    def reset_stats(self):
        L.check(self._lib.mk_reset_stats(self._h))

    # ---- index build (Miekki.cpp:277-314, 540-588)
    def insert_sequence(self, seq, title=""):
        """Miekki::insert_sequence (Miekki.cpp:243-273): one genome, its own size estimate (no u32 wrap of active^2)."""
        seq = bytes(seq)
        L.check(self._lib.mk_index_insert_sequence(self._h, seq, len(seq)))
        self.file_names.append(title)

    def index_file(self, path):
        """Miekki::index_file (Miekki.cpp:518-536): every non-header line of a (gzip'd) FASTA file as ONE genome."""
        import gzip
        import os
        if not os.path.exists(path):
            print(f"Missed file: {path}")
            return
        raw = open(path, "rb").read()
        if raw[:2] == b"\x1f\x8b":
            raw = gzip.decompress(raw)
        ref = b"".join(ln for ln in raw.split(b"\n") if not ln.startswith(b">"))
        if len(ref) >= self.kmer_size:
            self.insert_sequence(ref, path)

    def insert_sequences(self, seqs, names=None):
        seqs = [bytes(s) for s in seqs]
        if not seqs:
            return
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_index_append(self._h, ptrs, lens, len(seqs)))
        self.file_names += list(names) if names else [""] * len(seqs)

    def insert_sequences_packed(self, seqs, names=None):
        """insert_sequences for sequences handed over in the packed form of mk_index_append_packed
        (2-bit codes + exception bits + the first 32 characters): same index, a quarter of the bytes."""
        packed = [pack_sequence(bytes(s)) for s in seqs]
        if not packed:
            return
        arr = (L.PackedSeq * len(packed))()
        for i, (codes, exc, n, head) in enumerate(packed):
            arr[i].codes = codes.ctypes.data
            arr[i].except_ = exc.ctypes.data if exc is not None else None
            arr[i].len = n
            arr[i].head = head
        L.check(self._lib.mk_index_append_packed(self._h, arr, len(packed)))
        self.file_names += list(names) if names else [""] * len(packed)

    def insert_gz_files(self, blobs, names=None, fallback=True):
        """index_file_of_file's loop (Miekki.cpp:559-573) over gzip'd genome files whose BYTES are handed over: inflated,
        stripped of header lines and line feeds and appended on the device (mk_gz_unpack; the sequences never visit the
        host); a file the device refuses is inflated here (zstr's semantics: every member) when `fallback` is set.
        Returns the files' statuses (mk_gz_status).  Sequences shorter than k are skipped like the reference's."""
        blobs = [bytes(b) for b in blobs]
        n = len(blobs)
        if not n:
            return []
        ptrs, lens = L.seq_arrays(blobs)
        batch = C.c_void_p()
        L.check(self._lib.mk_gz_unpack(self._h, ptrs, lens, n, C.byref(batch)))
        status = []
        try:
            run, kept_names = [], []          # run: files of the batch waiting to be appended together
            def flush_run():
                for g0 in range(0, len(run), 64):
                    part = run[g0:g0 + 64]
                    L.check(self._lib.mk_index_append_gz(self._h, batch, (C.c_uint32 * len(part))(*part), len(part)))
                del run[:]
            for i in range(n):
                ln, st = C.c_uint64(), C.c_int32()
                L.check(self._lib.mk_gz_sequence(batch, i, C.byref(ln), C.byref(st)))
                status.append(st.value)
                if st.value == 0:
                    if ln.value >= self.kmer_size:
                        run.append(i); kept_names.append(names[i] if names else "")
                elif fallback:
                    ref = b"".join(l for l in _gunzip_members(blobs[i]).split(b"\n") if not l.startswith(b">"))
                    if len(ref) >= self.kmer_size:
                        flush_run()                       # (list order: the files before it first)
                        L.check(self._lib.mk_index_append(self._h, (C.c_char_p * 1)(ref), (C.c_uint64 * 1)(len(ref)), 1))
                        kept_names.append(names[i] if names else "")
            flush_run()
            L.check(self._lib.mk_sync(self._h))
            self.file_names += kept_names
        finally:
            self._lib.mk_gz_free(batch)
        return status

    def insert_synthetic(self, first_id, n, length):
        L.check(self._lib.mk_index_append_synthetic(self._h, first_id, n, length))
        self.file_names += [f"synthetic:{first_id + i}" for i in range(n)]

    def index_file_of_file(self, path, log=print):
        """Miekki.cpp:540-588 at -t 1: one path per line, <=3 character lines ignored,
        missing files reported, sequences shorter than k skipped, flush every 11."""
        if not os.path.exists(path):
            log(f"Missed file of file: {path}")
            return
        batch, names = [], []
        for fn in _read_text(path).split(b"\n"):
            if len(fn) <= 3:
                continue
            fn = fn.decode()
            if not os.path.exists(fn):
                log(f"Missed file: {fn}")
                continue
            ref = b"".join(l for l in _read_text(fn).split(b"\n") if not l.startswith(b">"))
            if len(ref) >= self.kmer_size:
                batch.append(ref); names.append(fn)
                if len(batch) > 10:
                    self.insert_sequences(batch, names)
                    batch, names = [], []
        self.insert_sequences(batch, names)
        log(f"Reference indexed: {self.index_size}")

    # ---- queries
    def query_sequences(self, seqs):
        """Miekki.cpp:344-372 -> uint32 [len(seqs), index_size]."""
        seqs = [bytes(s) for s in seqs]
        out = np.zeros((len(seqs), self.index_size), np.uint32)
        if seqs and self.index_size:
            ptrs, lens = L.seq_arrays(seqs)
            L.check(self._lib.mk_query_scores(self._h, ptrs, lens, len(seqs), out.ctypes.data))
        return out

    def query_sequence(self, seq):
        """Miekki.cpp:318-340 -> (scores[index_size], active_minimizer)."""
        hits, active = self.query([seq], 0, 0, 0.0)
        return self.query_sequences([seq])[0], int(active[0])

    def query(self, seqs, nresults=10, min_score=10, min_intersection=None):
        """filter_results(query_sequences(batch), ...) in one device pass
        (Miekki.cpp:437).  Returns (list of hit lists, active partitions)."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        seqs = [bytes(s) for s in seqs]
        nq = len(seqs)
        hits = (L.Hit * max(nq * max(nresults, 1), 1))()
        nhits = np.zeros(nq, np.uint32)
        active = np.zeros(nq, np.uint32)
        if nq:
            ptrs, lens = L.seq_arrays(seqs)
            L.check(self._lib.mk_query(self._h, ptrs, lens, nq, nresults, min_score, float(min_intersection),
                                       hits, nhits.ctypes.data, active.ctypes.data))
        out = []
        for q in range(nq):
            row = [hits[q * nresults + i] for i in range(int(nhits[q]))]
            out.append([SimilarityScore(h.genome, h.matches, h.jaccard, h.intersection) for h in row])
        return out, active

    def query_list(self, seqs, nresults=None, min_score=10, min_intersection=None):
        """filter_results(query_sequences(batch), nresults, ...) for any nresults in one device pass (mk_query_list);
        None: every genome above the thresholds.  Returns (list of hit lists, active partitions) like query()."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        seqs = [bytes(s) for s in seqs]
        nq = len(seqs)
        active = np.zeros(nq, np.uint32)
        if not nq:
            return [], active
        n = L.ALL_RESULTS if nresults is None else int(nresults)
        if nresults is not None and not 0 <= n < L.LIST_CANDIDATES:
            raise ValueError("nresults out of range")
        ptrs, lens = L.seq_arrays(seqs)
        hl = C.c_void_p()
        L.check(self._lib.mk_query_list(self._h, ptrs, lens, nq, n, min_score, float(min_intersection), C.byref(hl),
                                        active.ctypes.data))
        try:
            off = np.ctypeslib.as_array(self._lib.mk_hitlist_offsets(hl), (nq + 1,)).copy()
            total = int(off[nq])
            rec = np.zeros(total, _HIT_DTYPE)
            if total:
                C.memmove(rec.ctypes.data, self._lib.mk_hitlist_hits(hl), total * _HIT_DTYPE.itemsize)
        finally:
            self._lib.mk_hitlist_free(hl)
        rows = rec.tolist()
        return [[SimilarityScore(*r) for r in rows[int(off[q]):int(off[q + 1])]] for q in range(nq)], active

    def _hitlist(self, hl, nq):
        """a library-owned mk_hitlist -> list of hit lists (the list is freed)"""
        try:
            off = np.ctypeslib.as_array(self._lib.mk_hitlist_offsets(hl), (nq + 1,)).copy()
            total = int(off[nq])
            rec = np.zeros(total, _HIT_DTYPE)
            if total:
                C.memmove(rec.ctypes.data, self._lib.mk_hitlist_hits(hl), total * _HIT_DTYPE.itemsize)
        finally:
            self._lib.mk_hitlist_free(hl)
        rows = rec.tolist()
        return [[SimilarityScore(*r) for r in rows[int(off[q]):int(off[q + 1])]] for q in range(nq)]

    # ---- read pairs: the pair (seqs1[q], seqs2[q]) is ONE query (mk_qset_upload_pairs)
    @contextlib.contextmanager
    def pair_set(self, seqs1, seqs2):
        """The set of the pairs (seqs1[q], seqs2[q]) as a context manager: yields its handle for lib.mk_qset_run_* and the
        other mk_qset_* calls, and frees it.  A pair's k-mers are those of each mate alone; per partition the smallest
        fingerprint wins, mate 1 among equals, and the Bloom gate is asked for that winner (include/miekki_hip.h)."""
        seqs1, seqs2 = [bytes(s) for s in seqs1], [bytes(s) for s in seqs2]
        if len(seqs1) != len(seqs2):
            raise ValueError("read pairs need as many first mates as second mates: %d and %d" % (len(seqs1), len(seqs2)))
        p1, l1 = L.seq_arrays(seqs1)
        p2, l2 = L.seq_arrays(seqs2)
        qs = C.c_void_p()
        L.check(self._lib.mk_qset_upload_pairs(self._h, p1, l1, p2, l2, len(seqs1), C.byref(qs)))
        try:
            yield qs
        finally:
            self._lib.mk_qset_free(self._h, qs)

    def pair_scores(self, seqs1, seqs2):
        """query_sequences for read pairs (mk_qset_scores over pair_set) -> uint32 [n, index_size]."""
        with self.pair_set(seqs1, seqs2) as qs:
            n = len(seqs1)
            out = np.zeros((n, self.index_size), np.uint32)
            if out.size:
                d = C.c_void_p()
                L.check(self._lib.mk_dev_alloc(self._h, out.nbytes, C.byref(d)))
                try:
                    L.check(self._lib.mk_qset_scores(self._h, qs, 0, n, d))
                    L.check(self._lib.mk_sync(self._h))
                    L.check(self._lib.mk_dev_download(self._h, out.ctypes.data, d, out.nbytes))
                finally:
                    self._lib.mk_dev_free(self._h, d)
        return out

    def query_pairs(self, seqs1, seqs2, nresults=10, min_score=10, min_intersection=None):
        """query_list for read pairs (mk_qset_run_list and mk_qset_active over pair_set); nresults None: every genome above
        the thresholds.  Returns (list of hit lists, active partitions)."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        n = L.ALL_RESULTS if nresults is None else int(nresults)
        if nresults is not None and not 0 <= n < L.LIST_CANDIDATES:
            raise ValueError("nresults out of range")
        with self.pair_set(seqs1, seqs2) as qs:
            nq = len(seqs1)
            active = np.zeros(nq, np.uint32)
            if not nq:
                return [], active
            hl = C.c_void_p()
            L.check(self._lib.mk_qset_run_list(self._h, qs, n, min_score, float(min_intersection), C.byref(hl)))
            hits = self._hitlist(hl, nq)
            L.check(self._lib.mk_qset_active(self._h, qs, active.ctypes.data))
        return hits, active

    # ---- reads with base qualities: a read cut at its bad bases is ONE query (mk_qset_upload_reads)
    @contextlib.contextmanager
    def read_set(self, seqs, quals, min_qual, seqs2=None, quals2=None):
        """The set of the reads seqs[q] with the phred + 33 quality strings quals[q] as a context manager: yields its handle for
        lib.mk_qset_run_* and the other mk_qset_* calls, and frees it.  A base below min_qual (0 .. 93) cuts its read; the
        read's k-mers are those of each stretch of good bases alone, per partition the smallest fingerprint wins, the earliest
        stretch among equals, and the Bloom gate is asked for that winner (include/miekki_hip.h).  With seqs2 and quals2 the
        queries are pairs with qualities, as pair_set's."""
        seqs, quals = [bytes(s) for s in seqs], [bytes(s) for s in quals]
        if (seqs2 is None) != (quals2 is None):
            raise ValueError("second mates come with their qualities: seqs2 and quals2, both or neither")
        if len(seqs) != len(quals) or any(len(s) != len(x) for s, x in zip(seqs, quals)):
            raise ValueError("every read needs a quality string of its own length")
        if not 0 <= int(min_qual) <= 93:
            raise ValueError("min_qual out of range (0 .. 93)")
        p1, l1 = L.seq_arrays(seqs)
        x1, _ = L.seq_arrays(quals)
        p2 = l2 = x2 = None
        if seqs2 is not None:
            seqs2, quals2 = [bytes(s) for s in seqs2], [bytes(s) for s in quals2]
            if len(seqs2) != len(seqs):
                raise ValueError("read pairs need as many first mates as second mates: %d and %d" % (len(seqs), len(seqs2)))
            if len(seqs2) != len(quals2) or any(len(s) != len(x) for s, x in zip(seqs2, quals2)):
                raise ValueError("every read needs a quality string of its own length")
            p2, l2 = L.seq_arrays(seqs2)
            x2, _ = L.seq_arrays(quals2)
        qs = C.c_void_p()
        L.check(self._lib.mk_qset_upload_reads(self._h, p1, l1, x1, p2, l2, x2, len(seqs), int(min_qual), C.byref(qs)))
        try:
            yield qs
        finally:
            self._lib.mk_qset_free(self._h, qs)

    def read_scores(self, seqs, quals, min_qual, seqs2=None, quals2=None):
        """query_sequences for reads with qualities (mk_qset_scores over read_set) -> uint32 [n, index_size]."""
        with self.read_set(seqs, quals, min_qual, seqs2, quals2) as qs:
            n = len(seqs)
            out = np.zeros((n, self.index_size), np.uint32)
            if out.size:
                d = C.c_void_p()
                L.check(self._lib.mk_dev_alloc(self._h, out.nbytes, C.byref(d)))
                try:
                    L.check(self._lib.mk_qset_scores(self._h, qs, 0, n, d))
                    L.check(self._lib.mk_sync(self._h))
                    L.check(self._lib.mk_dev_download(self._h, out.ctypes.data, d, out.nbytes))
                finally:
                    self._lib.mk_dev_free(self._h, d)
        return out

    def query_reads(self, seqs, quals, min_qual, seqs2=None, quals2=None, nresults=10, min_score=10, min_intersection=None):
        """query_list for reads with qualities (mk_qset_run_list and mk_qset_active over read_set); nresults None: every
        genome above the thresholds.  Returns (list of hit lists, active partitions)."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        n = L.ALL_RESULTS if nresults is None else int(nresults)
        if nresults is not None and not 0 <= n < L.LIST_CANDIDATES:
            raise ValueError("nresults out of range")
        with self.read_set(seqs, quals, min_qual, seqs2, quals2) as qs:
            nq = len(seqs)
            active = np.zeros(nq, np.uint32)
            if not nq:
                return [], active
            hl = C.c_void_p()
            L.check(self._lib.mk_qset_run_list(self._h, qs, n, min_score, float(min_intersection), C.byref(hl)))
            hits = self._hitlist(hl, nq)
            L.check(self._lib.mk_qset_active(self._h, qs, active.ctypes.data))
        return hits, active

    def query_indexed(self, ids=None, nresults=10, min_score=10, min_intersection=None):
        """query_sequence(sequence of genome id) + filter_results for indexed genomes WITHOUT their sequences: a genome's
        stored column is its gated sketch (mk_qset_from_index).  ids: genome ids as the index reports them, any order
        (None: every genome, in id order); nresults None: every genome above the thresholds.  Returns (list of hit
        lists, active partitions) like query() / query_list()."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        base = self._p.genome_id_base
        ids = np.arange(base, base + self.index_size, dtype=np.uint32) if ids is None else np.ascontiguousarray(ids, np.uint32)
        n = L.ALL_RESULTS if nresults is None else int(nresults)
        if nresults is not None and not 0 <= n < L.LIST_CANDIDATES:
            raise ValueError("nresults out of range")
        active = np.zeros(len(ids), np.uint32)
        hits = []
        # sets of whole runs of 64 ids, as many as 2 GiB of query vectors and tables hold (3 bytes per partition and byte)
        per = max(64, min(4096, (2 << 30) // (3 * self.number_minimizer * self.W)) // 64 * 64)
        for i in range(0, len(ids), per):
            part = ids[i:i + per]
            qs, hl = C.c_void_p(), C.c_void_p()
            L.check(self._lib.mk_qset_from_index(self._h, part.ctypes.data, len(part), C.byref(qs)))
            try:
                L.check(self._lib.mk_qset_run_list(self._h, qs, n, min_score, float(min_intersection), C.byref(hl)))
                hits += self._hitlist(hl, len(part))
                L.check(self._lib.mk_qset_active(self._h, qs, active[i:].ctypes.data))
            finally:
                self._lib.mk_qset_free(self._h, qs)
        return hits, active

    def families(self, min_score=10, min_intersection=None):
        """The families the indexed genomes fall into (mk_index_families): genomes i and j are linked when either would be
        among the other's hits -- every genome above the thresholds, query_indexed(nresults=None) -- and a family is a
        connected component of the links.  Returns uint32 [index_size]: per genome the smallest genome id of its family,
        ids as the index reports them."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        labels = np.zeros(self.index_size, np.uint32)
        L.check(self._lib.mk_index_families(self._h, min_score, float(min_intersection), labels.ctypes.data))
        return labels

    def hierarchy(self, levels):
        """The nested families of the indexed genomes at several thresholds from one all-vs-all pass (mk_index_hierarchy).
        levels: (min_score, min_intersection) pairs, the loosest first, neither value falling from one to the next.  Returns
        uint32 [len(levels), index_size]: row l is what families(*levels[l]) returns, and every family of row l + 1 lies
        inside one family of row l."""
        levels = [(int(s), float(mi)) for s, mi in levels]
        arr = (L.Level * max(len(levels), 1))(*[L.Level(s, 0, mi) for s, mi in levels])
        labels = np.zeros((len(levels), self.index_size), np.uint32)
        L.check(self._lib.mk_index_hierarchy(self._h, arr, len(levels), labels.ctypes.data))
        return labels

    def representatives(self, min_score=10, min_intersection=None):
        """Greedy representative clustering of the indexed genomes in id order (mk_index_representatives), links as in
        families(): a genome is a representative unless an earlier representative is linked with it, and then belongs to
        the smallest such one.  Returns uint32 [index_size]: per genome the id of its representative (its own id: it is
        one), ids as the index reports them.  Earlier ids win: select() first for another priority."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        rep = np.zeros(self.index_size, np.uint32)
        L.check(self._lib.mk_index_representatives(self._h, min_score, float(min_intersection), rep.ctypes.data))
        return rep

    def tally(self, seqs, min_score=10, min_intersection=None):
        """The profile of a read set (mk_query_tally): per indexed genome, how many of the sequences list it -- it is among
        query_list(nresults=None) -- how many list it alone, for how many it is the best hit -- query_list(nresults=1) --
        and the matches of those.  Nothing per sequence comes back from the device.  Returns uint64 [index_size, 4]:
        listed, unique, best, best_matches per local genome."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        seqs = [bytes(s) for s in seqs]
        out = np.zeros((self.index_size, 4), np.uint64)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_tally(self._h, ptrs, lens, len(seqs), min_score, float(min_intersection), out.ctypes.data))
        return out

    def clade_tally(self, seqs, clades, min_score=10, min_intersection=None):
        """The profile of a read set by clade (mk_query_clade_tally): `clades` gives every local genome its clade number
        (index_size integers; None or -1: the genome is left out of the pass), non-decreasing among the genomes that have
        one -- the layout select() with a families list produces.  Returns uint64 [n_clades, 5], n_clades = 1 + the largest
        number given: listed (sequences that list a member, once each), unique (that list members of this clade only), best
        (whose best hit among the genomes with a clade is a member), best_matches, hits (sequence-member pairs)."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        seqs = [bytes(s) for s in seqs]
        given = [-1 if c is None else int(c) for c in clades]
        if len(given) != self.index_size:
            raise ValueError(f"{len(given)} clade numbers for {self.index_size} genomes")
        if any(c < -1 or c >= L.NO_CLADE for c in given):
            raise ValueError("clade numbers are 0 .. 2^32 - 2, or None / -1 for a genome that is left out")
        n_clades = 1 + max(given, default=-1)
        cl = np.array([L.NO_CLADE if c < 0 else c for c in given], np.uint32)
        out = np.zeros((n_clades, 5), np.uint64)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_clade_tally(self._h, ptrs, lens, len(seqs), min_score, float(min_intersection), cl.ctypes.data,
                                               n_clades, out.ctypes.data))
        return out

    def lca(self, seqs, nodes, margin=100, min_score=10, min_intersection=None, per_read=False):
        """Every sequence placed in a taxonomy by lowest common ancestor (mk_query_lca).  `nodes` is a sequence of (lo, hi):
        nested intervals [lo, hi) of local genome ids in preorder -- a parent before its children, by ascending lo; genomes
        inside no node are left out of the pass.  A sequence belongs to the deepest node that holds every genome it lists
        whose intersection is within `margin` percent of its best one's (100: all of them, 0: the ties with the best).
        Returns uint64 [n_nodes + 1, 3] -- reads, best_matches, hits per node, the last row for the sequences above every
        node -- and with per_read also uint32 [len(seqs)]: each sequence's node, lib.LCA_ABOVE, or lib.NO_NODE for one that
        lists nothing."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or not 0 <= margin <= 100:
            raise ValueError("the margin is an integer percentage, 0 .. 100")
        lo, hi = _node_arrays(nodes)
        seqs = [bytes(s) for s in seqs]
        n_nodes = len(lo)
        out = np.zeros((n_nodes + 1, 3), np.uint64)
        node = np.full(len(seqs), L.NO_NODE, np.uint32)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_lca(self._h, ptrs, lens, len(seqs), min_score, float(min_intersection), int(margin), lo.ctypes.data,
                                       hi.ctypes.data, n_nodes, out.ctypes.data, node.ctypes.data if per_read else None))
        return (out, node) if per_read else out

    def abundance(self, seqs, rounds=50, margin=100, min_score=10, min_intersection=None, shift=None):
        """How many of the sequences each genome gets, by expectation-maximisation over the ones that several genomes share
        (mk_query_abundance; with a `shift`: mk_share_create, mk_qset_run_share, mk_share_rounds).  A sequence whose genomes
        within `margin` percent of its best one are several is split among them in proportion to the weights of the round
        before, `rounds` times, from equal weights.  Returns (abundance, unique, shared, info, result): uint64 [index_size]
        each -- abundance in reads with 32 fractional bits --, info = {queries, assigned, shared_reads, entries}, result =
        {delta, starved, rounds, shift}.  Genome length plays no part: the abundances are fractions of reads, not coverage."""
        if min_intersection is None:
            min_intersection = 0.5 * self.threshold
        if isinstance(margin, bool) or not isinstance(margin, (int, np.integer)) or not 0 <= margin <= 100:
            raise ValueError("the margin is an integer percentage, 0 .. 100")
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= rounds < 2 ** 32:
            raise ValueError("the rounds are an integer from 1 on")
        if shift is not None and (isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or not 0 <= shift <= 32):
            raise ValueError("the shift is an integer, 0 .. 32, or None for the smallest that fits")
        seqs = [bytes(s) for s in seqs]
        G = self.index_size
        a, u, s = (np.zeros(G, np.uint64) for _ in range(3))
        info, res = L.ShareInfo(), L.ShareResult()
        ptrs, lens = L.seq_arrays(seqs)
        if shift is None:
            L.check(self._lib.mk_query_abundance(self._h, ptrs, lens, len(seqs), min_score, float(min_intersection), int(margin), int(rounds),
                                                 a.ctypes.data, u.ctypes.data, s.ctypes.data, C.byref(info), C.byref(res)))
        else:
            pool, qs = C.c_void_p(), C.c_void_p()
            L.check(self._lib.mk_share_create(self._h, C.byref(pool)))
            try:
                L.check(self._lib.mk_qset_upload(self._h, ptrs, lens, len(seqs), C.byref(qs)))
                try:
                    L.check(self._lib.mk_qset_run_share(self._h, qs, min_score, float(min_intersection), int(margin), pool))
                finally:
                    self._lib.mk_qset_free(self._h, qs)
                L.check(self._lib.mk_share_rounds(self._h, pool, int(rounds), int(shift), a.ctypes.data, C.byref(res)))
                L.check(self._lib.mk_share_export(self._h, pool, u.ctypes.data, s.ctypes.data, None, None))
                L.check(self._lib.mk_share_info_read(self._h, pool, C.byref(info)))
            finally:
                self._lib.mk_share_free(self._h, pool)
        return (a, u, s, {f[0]: int(getattr(info, f[0])) for f in L.ShareInfo._fields_},
                {f[0]: int(getattr(res, f[0])) for f in L.ShareResult._fields_})

    def cover(self, seqs):
        """Breadth of coverage (mk_query_cover): per indexed genome, how many of its stored fingerprints turn up in the gated
        sketch of at least one of the sequences -- one pass over the matrix whatever their number, no thresholds.  Returns
        (uint32 [index_size], cells): covered per local genome, and the (partition, value) cells the sequences mark.  With
        8-bit fingerprints an unrelated genome is covered at about cells / (2^h * 256) of its sketch by chance."""
        seqs = [bytes(s) for s in seqs]
        out = np.zeros(self.index_size, np.uint32)
        cells = C.c_uint64(0)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_cover(self._h, ptrs, lens, len(seqs), out.ctypes.data, C.byref(cells)))
        return out, int(cells.value)

    def taxon_cover(self, seqs, nodes):
        """Distinct covered cells per node of a taxonomy (mk_query_taxonomy_cover).  `nodes` is what lca() takes.  Per node: held,
        the distinct (partition, value) cells its genomes hold -- a cell that sixty-four strains share counts once --, and
        covered, those of them the gated sketch of at least one of the sequences holds.  A node of one genome has that
        genome's sketch_size and cover() count, a root over all genomes cover_winners()' claimed.  Returns (uint64
        [n_nodes, 2]: held, covered per node; cells); read covered / held against cells / (2^h * 256) as for cover()."""
        lo, hi = _node_arrays(nodes)
        seqs = [bytes(s) for s in seqs]
        out = np.zeros((len(lo), 2), np.uint64)
        cells = C.c_uint64(0)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_taxonomy_cover(self._h, ptrs, lens, len(seqs), lo.ctypes.data, hi.ctypes.data, len(lo),
                                                  out.ctypes.data, C.byref(cells)))
        return out, int(cells.value)

    def markers(self, seqs, nodes):
        """Taxon-specific cells (mk_query_taxonomy_markers).  `nodes` is what lca() takes.  Every held cell belongs to the deepest
        node that contains all its holders (genomes inside no node left out); per node: specific, the cells it owns, and
        covered, those of them the gated sketch of at least one of the sequences holds.  The last row is the slot above every
        node.  Subtree sums over lca's parents give the cells held inside a node and nowhere outside it.  `seqs=None`: specific
        alone, no table (mk_taxonomy_markers with a NULL table).  Returns (uint64 [n_nodes + 1, 2]: specific, covered; cells)."""
        lo, hi = _node_arrays(nodes)
        out = np.zeros((len(lo) + 1, 2), np.uint64)
        cells = C.c_uint64(0)
        if seqs is None:
            tax = C.c_void_p()
            L.check(self._lib.mk_taxonomy_create(self._h, lo.ctypes.data, hi.ctypes.data, len(lo), self.index_size, C.byref(tax)))
            try:
                L.check(self._lib.mk_taxonomy_markers(self._h, tax, None, out.ctypes.data, len(out), C.byref(cells)))
            finally:
                self._lib.mk_taxonomy_free(self._h, tax)
            return out, int(cells.value)
        seqs = [bytes(s) for s in seqs]
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_taxonomy_markers(self._h, ptrs, lens, len(seqs), lo.ctypes.data, hi.ctypes.data, len(lo),
                                                    out.ctypes.data, len(out), C.byref(cells)))
        return out, int(cells.value)

    def cover_winners(self, seqs):
        """The winner-takes-all screen (mk_query_cover_winners): the count of cover(), and then every seen cell that some
        genome holds credited to ONE of its holders -- the first in the order by share of its own sketch covered, then covered,
        then id -- so that a strain that is present keeps its cells and its relatives keep what they alone explain.  One
        round: the order comes from the plain counts.  Returns (covered, won, cells, claimed): uint32 [index_size] each per
        local genome, the cells the sequences mark, and those of them some genome holds (= won.sum())."""
        seqs = [bytes(s) for s in seqs]
        covered, won = np.zeros(self.index_size, np.uint32), np.zeros(self.index_size, np.uint32)
        cells, claimed = C.c_uint64(0), C.c_uint64(0)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_cover_winners(self._h, ptrs, lens, len(seqs), covered.ctypes.data, won.ctypes.data,
                                                 C.byref(cells), C.byref(claimed)))
        return covered, won, int(cells.value), int(claimed.value)

    def depth(self, seqs):
        """Depth of coverage (mk_query_depth): per indexed genome, over the stored fingerprints that the gated sketch of at
        least one of the sequences holds, in how many of the sequences each turns up -- capped at 255 -- as the lower median
        and the sum; nine passes over the matrix whatever their number, integers only.  Returns (median uint32 [index_size],
        sum uint64 [index_size], covered uint32 [index_size], cells, saturated): per local genome; the (partition, value)
        cells the sequences mark, and those of them at the cap (a median of 255 means "255 or more").  The mean depth is
        sum / covered.  With 8-bit fingerprints read a median only where covered / sketch_size stands clear of
        cells / (2^h * 256)."""
        seqs = [bytes(s) for s in seqs]
        out = np.zeros(self.index_size, np.dtype([("sum", np.uint64), ("covered", np.uint32), ("median", np.uint32)]))
        cells, saturated = C.c_uint64(0), C.c_uint64(0)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_depth(self._h, ptrs, lens, len(seqs), out.ctypes.data, C.byref(cells), C.byref(saturated)))
        return out["median"].copy(), out["sum"].copy(), out["covered"].copy(), int(cells.value), int(saturated.value)

    def panel(self, samples):
        """The cover of a cohort (mk_query_panel): `samples` is a sequence of samples, each a sequence of byte strings; eight
        samples share one table and ONE pass over the matrix -- a bit of the table's byte each -- so n samples cost ceil(n / 8)
        passes where cover() costs n.  Returns (covered uint32 [n_samples, index_size], cells uint64 [n_samples]): row s is
        what cover(samples[s]) returns, count for count."""
        samples = [[bytes(q) for q in sample] for sample in samples]
        seqs = [q for sample in samples for q in sample]
        starts = np.zeros(len(samples) + 1, np.uint64)
        starts[1:] = np.cumsum([len(sample) for sample in samples], dtype=np.uint64)
        covered = np.zeros((len(samples), self.index_size), np.uint32)
        cells = np.zeros(len(samples), np.uint64)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_panel(self._h, ptrs, lens, starts.ctypes.data, len(samples), covered.ctypes.data, cells.ctypes.data))
        return covered, cells

    PICK_DTYPE = np.dtype([("genome", np.uint32), ("fresh", np.uint32), ("covered", np.uint32), ("sketch_size", np.uint32),
                           ("depth_sum", np.uint64)])

    def gather(self, seqs, min_new=10, max_picks=0, depth=False):
        """The greedy gather (mk_query_cover_gather; sourmash's gather): the genome that explains most of the cells the
        sequences mark, those cells struck from the sample, and again on what is left -- until no genome explains min_new
        cells, or max_picks genomes are picked (0: no cap).  Among equals the smallest id wins.  Returns (picks, cells,
        explained): picks is a structured array in pick order with the fields of mk_pick -- genome (the reported id), fresh
        (what the pick explains that none before it did), covered (its overlap with the whole sample), sketch_size and
        depth_sum (depth=True: the sum over the struck cells of the sequences that hold each, capped at 255 per cell; else 0)
        -- cells the cells the sequences mark, explained the sum of fresh.  With 8-bit fingerprints an unrelated genome's fresh
        is about sketch_size * live cells / (2^h * 256): min_new has to stand clear of it."""
        seqs = [bytes(s) for s in seqs]
        room = min(int(max_picks), self.index_size) if max_picks else self.index_size
        out = np.zeros(max(room, 1), self.PICK_DTYPE)
        n, cells, explained = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        ptrs, lens = L.seq_arrays(seqs)
        L.check(self._lib.mk_query_cover_gather(self._h, ptrs, lens, len(seqs), 1 if depth else 0, int(min_new), int(max_picks),
                                                out.ctypes.data, C.byref(n), C.byref(cells), C.byref(explained)))
        return out[:n.value].copy(), int(cells.value), int(explained.value)

    def query_index_file(self, out, names=None, nresults=10):
        """The all-vs-all of `miekki -X`: every indexed genome against the index, one line of query_whole_file's format
        (Miekki.cpp:503-509) per genome that has hits, in id order.  names: what a line starts with, per genome (the
        file names when the index was built from a list); None: the genome ids in decimal."""
        hits, _ = self.query_indexed(None, nresults, 10, 0.5 * self.threshold)
        base = self._p.genome_id_base
        for g, row in enumerate(hits):
            if row:
                name = names[g] if names is not None else b"%d" % (g + base)
                out.write(self.format_hits(name if isinstance(name, bytes) else str(name).encode(), row))

    def filter_results(self, scores, nresults, min_score, min_intersection):
        """Miekki.cpp:376-422 over host scores (a row or a matrix)."""
        scores = np.asarray(scores, np.uint32)
        if scores.ndim == 2:
            return [self.filter_results(r, nresults, min_score, min_intersection) for r in scores]
        ss, gs = self.sketch_size, self.genome_size
        with np.errstate(divide="ignore", invalid="ignore"):
            jac = scores.astype(np.float64) / ss
            inter = jac * gs
        keep = np.flatnonzero((scores >= min_score) & ~(inter < min_intersection))
        cand = (L.Hit * max(len(keep), 1))()
        for i, g in enumerate(keep):
            cand[i] = L.Hit(int(g) + self._p.genome_id_base, int(scores[g]), float(jac[g]), float(inter[g]))
        out = (L.Hit * max(nresults, 1))()
        n = self._lib.mk_filter_candidates(cand, len(keep), nresults, out)
        return [SimilarityScore(out[i].genome, out[i].matches, out[i].jaccard, out[i].intersection) for i in range(n)]

    @staticmethod
    def format_hits(name: bytes, hits) -> bytes:
        """One output line of query_file (Miekki.cpp:440-444)."""
        return name + b":" + b"".join(
            b"%d\t%d\t%d\t%s;" % (h.genome, h.matches, int(h.intersection), ("%f" % h.jaccard).encode())
            for h in hits) + b"\n"

    def query_file(self, path, out, batch_size=4096, nresults=10):
        """Miekki.cpp:426-483 at -t 1: strict 2-line records, records shorter than k
        skipped, one line per kept record.  nresults: the reference's ten, any other number, or None for
        every genome above the thresholds (query_list)."""
        if not os.path.exists(path):
            print("File problem")
            return
        lines = _read_text(path).split(b"\n")
        recs = [(lines[i], lines[i + 1] if i + 1 < len(lines) else b"") for i in range(0, len(lines), 2)]
        recs = [(h, s) for h, s in recs if len(s) >= self.kmer_size]
        for i in range(0, len(recs), batch_size):
            chunk = recs[i:i + batch_size]
            if nresults == 10:
                hits, _ = self.query([s for _, s in chunk], 10, 10, 0.5 * self.threshold)
            else:
                hits, _ = self.query_list([s for _, s in chunk], nresults, 10, 0.5 * self.threshold)
            out.write(b"".join(self.format_hits(h, r) for (h, _), r in zip(chunk, hits)))

    # ---- exact mode (Miekki.cpp:792-859)
    def ground_truth_batch(self, queries, fasta: bytes):
        """|A n B| and |A u B| of each query against the genome file's k-mer set."""
        k = self.kmer_size
        contigs, ref = [], b""
        for line in fasta.split(b"\n"):
            if line.startswith(b">"):
                if len(ref) >= k:                       # short contigs leak into the next (806-812)
                    contigs.append(ref); ref = b""
            else:
                ref += line
        if len(ref) >= k:
            contigs.append(ref)
        queries = [bytes(q) for q in queries]
        cp, cl = L.seq_arrays(contigs)
        qp, ql = L.seq_arrays(queries)
        inter = np.zeros(len(queries), np.uint64)
        uni = np.zeros(len(queries), np.uint64)
        L.check(self._lib.mk_exact(self._h, cp, cl, len(contigs), qp, ql, len(queries),
                                   inter.ctypes.data, uni.ctypes.data))
        return inter, uni

    # ---- persistence (Miekki.cpp:649-719)
    def serialize(self, chunk_rows=4096):
        """Yield the uncompressed index stream piecewise."""
        G, W, P = self.index_size, self.W, self.number_minimizer
        yield _HDR.pack(self._p.k, self._p.h, self._p.fp_bits, 5, G, self._p.bloom_log2, self.bloom_size,
                        0, 0, self._p.threshold, 1)
        rows = max(1, min(P, (64 << 20) // max(G * W, 1)))
        buf = np.empty(rows * G * W, np.uint8)
        for p in range(0, P, rows):
            r = min(rows, P - p)
            if G:
                L.check(self._lib.mk_index_export_columns(self._h, p, p + r, buf.ctypes.data))
            yield buf[:r * G * W].tobytes()
        yield self.genome_size.tobytes()
        nb = self.bloom_size // 8
        step = 64 << 20
        b = np.empty(min(step, max(nb, 1)), np.uint8)
        for o in range(0, nb, step):
            e = min(nb, o + step)
            L.check(self._lib.mk_index_export_bloom(self._h, o, e, b.ctypes.data))
            yield b[:e - o].tobytes()
        yield self.sketch_size.tobytes()

    def dump_disk(self, path):
        """gzip level 1 like zstr::ofstream (zstr.hpp:82,230)."""
        with gzip.open(path, "wb", compresslevel=1) as f:
            for piece in self.serialize():
                f.write(piece)

    @classmethod
    def load(cls, path, device=0, genome_id_base=0):
        """Miekki(const string& input), Miekki.cpp:682-719; gzip or plain like zstr::ifstream."""
        if not os.path.exists(path):
            raise FileNotFoundError("File problem")
        with open(path, "rb") as raw:
            magic = raw.read(2)
        f = gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")
        with f:
            k, h, fpb, _nbm, G, bl2, bbits, _jac, _cont, thr, _comp = _HDR.unpack(_readn(f, 39))
            ix = cls(k, h, fpb, bl2, thr, device, genome_id_base)
            W, P = fpb // 8, 1 << h
            L.check(ix._lib.mk_index_import_begin(ix._h, G))
            rows = max(1, min(P, (64 << 20) // max(G * W, 1)))
            for p in range(0, P, rows):
                r = min(rows, P - p)
                buf = _readn(f, r * G * W)
                if G:
                    L.check(ix._lib.mk_index_import_columns(ix._h, p, p + r, buf))
            gs = np.frombuffer(_readn(f, 8 * G), np.uint64)
            nb, step = bbits // 8, 64 << 20
            for o in range(0, nb, step):
                e = min(nb, o + step)
                L.check(ix._lib.mk_index_import_bloom(ix._h, o, e, _readn(f, e - o)))
            ss = np.frombuffer(_readn(f, 4 * G), np.uint32)
            L.check(ix._lib.mk_index_import_sizes(ix._h, gs.ctypes.data if G else None, ss.ctypes.data if G else None)
                    if G else 0)
        return ix


def pack_sequence(seq: bytes, piece=None):
    """(codes uint64[], except uint64[] or None, len, head) of mk_packed_seq through the library's own
    host packer, mk_pack_append -- in `piece`-sized appends when given (a reader packs line by line)."""
    lib = L.load_library()
    n = len(seq)
    codes = np.zeros(lib.mk_pack_code_words(n), np.uint64)
    exc = np.zeros(lib.mk_pack_except_words(n), np.uint64)
    dirty = 0
    step = piece or max(n, 1)
    for at in range(0, n, step):
        chunk = seq[at:at + step]
        rc = lib.mk_pack_append(codes.ctypes.data, exc.ctypes.data, at, chunk, len(chunk))
        if rc < 0:
            raise ValueError("mk_pack_append failed")
        dirty |= rc
    return codes, (exc if dirty else None), n, seq[:32]


def _readn(f, n):
    b = f.read(n)
    if len(b) != n:
        raise EOFError("truncated index stream")
    return b


def _gunzip_members(data: bytes) -> bytes:
    """every gzip member from the start; what follows the last whole member is ignored (zlib's gzread does the same)"""
    import zlib
    out = []
    while data[:2] == b"\x1f\x8b":
        d = zlib.decompressobj(31)
        try:
            out.append(d.decompress(data))
        except zlib.error:
            break
        if not d.eof:
            break
        data = d.unused_data
    return b"".join(out)


def _read_text(path) -> bytes:
    """Whole file, gunzipped when it starts with the gzip magic (zstr.hpp:157-167)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)          # every member, like zstr (zstr.hpp:186-190)
    return data
