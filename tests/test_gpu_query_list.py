"""Every genome above the thresholds, not only the best ten: mk_query_list / Miekki.query_list / `miekki -n`.

The contract is Miekki::filter_results(row, N, min_score, min_intersection) (Miekki.cpp:376-397) for any N -- N = index
size for "every genome" -- ties included.  Every comparison below is with the CPU oracle built from the same sequences:
exact equality of (genome, matches, jaccard, intersection) and of the order, for every query of every case."""
import os
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "miekki_amd", "miekki")

# The strain families (the case the lists exist for): 5 species x 96 strains of 100 kb at -k 31 -h 14, 3,000 substitutions
# per million bases, threshold 200 (min_intersection 100), 1 kb queries cut from strains.  Chosen on the CPU: of the 640
# queries below the oracle keeps between 96 and 250 genomes each (mean 116) -- every one more than 64 and more than 65.
SP, ST, SL, PPM, SK, SH, STHR = 5, 96, 100_000, 3000, 31, 14, 200
NS = [None, 65, 100, 1000]


@pytest.fixture(scope="module")
def hip():
    import miekki_amd
    return miekki_amd


def want_lists(o, rows, N, ms, mi):
    n = o.index_size if N is None else N
    return [o.filter_results(r, n, ms, mi) for r in rows]


def assert_same(got, want):
    assert len(got) == len(want)
    for q in range(len(want)):
        assert [tuple(x) for x in got[q]] == want[q], q


def cut_queries(seqs, n, seed, qlen=1000):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        g = int(rng.integers(0, len(seqs)))
        off = int(rng.integers(0, len(seqs[g]) - qlen))
        out.append(seqs[g][off:off + qlen])
    return out


@pytest.fixture(scope="module")
def strains(hip):
    from oracle import oracle as orc
    G = SP * ST
    seqs = [synth.strain_device(g, ST, PPM, 0, SL) for g in range(G)]
    o = orc.OracleMiekki(SK, SH, 8, 33, STHR)
    o.insert_sequences(seqs)
    ix = hip.Miekki(SK, SH, 8, 33, STHR)
    for g0 in range(0, G, 48):
        ix.insert_sequences(seqs[g0:g0 + 48])
    big = cut_queries(seqs, 640, 11)
    rows = o.query_sequences(big)
    yield ix, o, seqs, big, rows
    ix.close()


def test_strain_preconditions_from_the_oracle_alone(strains):
    _, o, _, _, rows = strains
    passing = [len(w) for w in want_lists(o, rows, None, 10, 0.5 * STHR)]
    assert max(passing) > 64                      # the no-eviction sequence beyond the old device limit
    assert sum(p > 65 for p in passing) >= 1      # and the eviction sequence for N = 65
    assert sum(p > 100 for p in passing) >= 1


@pytest.mark.parametrize("N", NS)
def test_strain_families_slab_schedule(strains, monkeypatch, N):
    ix, o, _, big, rows = strains
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "4")    # four partition ranges at -h 14: 640 queries take the range-table schedule
    before = ix.stats()
    got, act = ix.query_list(big, N)
    after = ix.stats()
    assert after["scan_slab_launches"] > before["scan_slab_launches"]
    assert after["scan_launches"] - before["scan_launches"] == after["scan_slab_launches"] - before["scan_slab_launches"]
    assert_same(got, want_lists(o, rows, N, 10, 0.5 * STHR))
    assert [int(a) for a in act[:24]] == [o.query_sequence(s)[1] for s in big[:24]]


@pytest.mark.parametrize("N", NS)
def test_strain_families_small_set(strains, N):
    ix, o, _, big, rows = strains
    got, _ = ix.query_list(big[100:300], N)       # below 512 queries: ranges cut by count
    assert_same(got, want_lists(o, rows[100:300], N, 10, 0.5 * STHR))


def test_equivalence_with_the_paths_that_exist(strains):
    ix, _, _, big, _ = strains
    qs = big[:150]
    for N in (10, 64):
        assert ix.query_list(qs, N)[0] == ix.query(qs, N)[0]            # the old device heap
    assert ix.query_list(qs[:40], 100)[0] == ix.query(qs[:40], 100)[0]  # mk_query's per-query fallback
    assert ix.query_list(qs[:8], 0)[0] == [[] for _ in range(8)]


@pytest.mark.parametrize("kib", [1, 16])
def test_chunk_cut_into_runs_by_a_small_record_budget(strains, monkeypatch, kib):
    """1 KiB = 128 records: fewer than any query of the set leaves, so every query is a run of its own; 16 KiB: runs of
    several queries.  Same answer."""
    ix, o, _, big, rows = strains
    monkeypatch.setenv("MIEKKI_LIST_BUDGET_KIB", str(kib))
    for N in (None, 65):
        got, _ = ix.query_list(big[:90], N)
        assert_same(got, want_lists(o, rows[:90], N, 10, 0.5 * STHR))


def test_whole_genomes_long_reads_and_mixed_sets(strains):
    """the dense schedule (whole genomes, -A), the sparse long path, and a mixed set that is split in two"""
    ix, o, seqs, big, _ = strains
    whole = [seqs[3], seqs[200], seqs[479]]
    longr = [seqs[7][:9000], seqs[300][5000:25_000]]
    nohit = [synth.genome_bases(4_000_000, 0, 1000)]
    for qs in (whole, longr, [big[0], whole[0], big[1], longr[0], nohit[0], big[2], whole[1]]):
        rows = o.query_sequences(qs)
        for N in (None, 65):
            got, _ = ix.query_list(qs, N)
            assert_same(got, want_lists(o, rows, N, 10, 0.5 * STHR))
    got, act = ix.query_list(nohit)
    assert got == [[]] and len(act) == 1
    got, act = ix.query_list([])
    assert got == [] and len(act) == 0


def test_second_slice_of_mk_query_list(strains):
    """2^18 + 5 reads, 64 distinct ones repeated: mk_query_list takes them as two uploaded sets and the second one's lists go
    behind the first one's -- query i has the oracle's list of read i mod 64, the offsets are the lists' running sum.
    Thresholds chosen on the CPU for reads of 100 bases (70 k-mers): at (5, 30.0) the oracle keeps between 20 and 99 genomes
    for each of the 64, so the best three of each are what a heap with evictions leaves."""
    import ctypes as C
    from miekki_amd import lib as L
    ix, o, seqs, _, _ = strains
    N, ms, mi = 3, 5, 30.0
    reads, queries, _ = synth.two_slices(seqs, 23)
    nq = len(queries)
    assert nq == (1 << 18) + 5
    hit = np.dtype([("genome", "<u4"), ("matches", "<u4"), ("jaccard", "<f8"), ("intersection", "<f8")])
    assert hit.itemsize == C.sizeof(L.Hit)
    rows = o.query_sequences(reads)
    assert min(len(w) for w in want_lists(o, rows, None, ms, mi)) >= 20
    each = [np.array(w, hit) for w in want_lists(o, rows, N, ms, mi)]
    assert all(len(w) == N for w in each) and len({int(g) for w in each for g in w["genome"]}) >= 2    # (on the oracle: nothing passes on zeros)
    want_off = np.concatenate([[0], np.cumsum([len(each[i % 64]) for i in range(nq)])]).astype(np.uint64)
    ptrs, lens = L.seq_arrays(queries)
    hl, active = C.c_void_p(), np.zeros(nq, np.uint32)
    L.check(ix._lib.mk_query_list(ix._h, ptrs, lens, nq, N, ms, mi, C.byref(hl), active.ctypes.data))
    try:
        off = np.ctypeslib.as_array(ix._lib.mk_hitlist_offsets(hl), (nq + 1,)).copy()
        np.testing.assert_array_equal(off, want_off)
        got = np.zeros(int(off[nq]), hit)
        C.memmove(got.ctypes.data, ix._lib.mk_hitlist_hits(hl), got.nbytes)
    finally:
        ix._lib.mk_hitlist_free(hl)
    assert got.tobytes() == np.concatenate([each[i % 64] for i in range(nq)]).tobytes()
    want_act = [o.query_sequence(r)[1] for r in reads]
    np.testing.assert_array_equal(active, np.array([want_act[i % 64] for i in range(nq)], np.uint32))


def test_empty_index(hip):
    ix = hip.Miekki(21, 12, 8, 32, 20)
    try:
        got, act = ix.query_list([synth.genome_bases(1, 0, 500), synth.genome_bases(2, 0, 9000)])
        assert got == [[], []] and list(act) == [0, 0]
    finally:
        ix.close()


def build_pair(hip, case):
    from oracle import oracle as orc
    seqs = case.genome_sequences()
    o = orc.OracleMiekki(case.k, case.h, case.fp_bits, case.b, case.threshold)
    o.insert_sequences(seqs)
    ix = hip.Miekki(case.k, case.h, case.fp_bits, case.b, case.threshold)
    ix.insert_sequences(seqs)
    return ix, o


def test_ties_duplicate_genomes(hip):
    """three hundred copies of one genome: equal intersections, ordered as the reference's heap calls order them"""
    case = synth.case_dups()
    ix, o = build_pair(hip, case)
    try:
        qs = [s for _, s in case.query_sequences()]
        rows = o.query_sequences(qs)
        full = want_lists(o, rows, None, 10, 0.5 * case.threshold)
        assert max(len(w) for w in full) >= 300
        for N in (None, 150, 299, 65):            # 150, 299, 65: cuts through the group of 300 equals
            got, _ = ix.query_list(qs, N, 10, 0.5 * case.threshold)
            assert_same(got, want_lists(o, rows, N, 10, 0.5 * case.threshold))
    finally:
        ix.close()


def test_ties_equal_sizes_poked(hip):
    """genomes of one size poked with equal sketch and genome sizes: equal scores are equal intersections"""
    from oracle import oracle as orc
    from miekki_amd import lib as L
    k, h, G = 21, 12, 160
    seqs = [synth.strain_device(g, 80, 500, 0, 30_000) for g in range(G)]
    o = orc.OracleMiekki(k, h, 8, 32, 20)
    o.insert_sequences(seqs)
    ix = hip.Miekki(k, h, 8, 32, 20)
    try:
        ix.insert_sequences(seqs)
        ss, gs = np.full(G, 3000, np.uint32), np.full(G, 30_000, np.uint64)
        o.poke_sizes(ss, gs)
        L.check(ix._lib.mk_index_import_sizes(ix._h, gs.ctypes.data, ss.ctypes.data))
        qs = cut_queries(seqs, 60, 5, 700)
        rows = o.query_sequences(qs)
        full = want_lists(o, rows, None, 10, 10.0)
        inters = [w[3] for w in full[0]]
        assert len(inters) > len(set(inters)) and max(len(w) for w in full) > 64     # tie groups, beyond the old limit
        for N in (None, 70, 33):
            got, _ = ix.query_list(qs, N, 10, 10.0)
            assert_same(got, want_lists(o, rows, N, 10, 10.0))
    finally:
        ix.close()


def test_two_byte_fingerprints(hip):
    case = synth.case_w16()
    ix, o = build_pair(hip, case)
    try:
        qs = [s for _, s in case.query_sequences()]
        rows = o.query_sequences(qs)
        for N, ms, mi in ((None, 10, 0.5 * case.threshold), (None, 1, 0.0), (3, 1, 0.0)):
            got, _ = ix.query_list(qs, N, ms, mi)
            assert_same(got, want_lists(o, rows, N, ms, mi))
    finally:
        ix.close()


def test_cold_rows_under_a_small_hbm_budget(hip, monkeypatch):
    """rows beyond a 1 MiB budget live in host memory; 700 queries stream the cold ranges (the slab schedule), a handful
    read them in place, long queries take the row windows.  Low thresholds: hundreds of genomes pass by chance."""
    from oracle import oracle as orc
    k, h, G = 21, 12, 600
    seqs = [synth.genome_bases(9000 + g, 0, 12_000 + 37 * (g % 600)) for g in range(G)]
    monkeypatch.setenv("MIEKKI_SLAB_MIB", "1")
    monkeypatch.setenv("MIEKKI_HBM_MATRIX_MIB", "1")
    o = orc.OracleMiekki(k, h, 8, 32, 10)
    o.insert_sequences(seqs)
    ix = hip.Miekki(k, h, 8, 32, 10)
    try:
        for i in range(0, G, 150):
            ix.insert_sequences(seqs[i:i + 150])
        rng = np.random.default_rng(77)
        qs = []
        for q in range(700):
            g = int(rng.integers(0, G))
            off = int(rng.integers(0, len(seqs[g]) - 1300))
            qs.append(seqs[g][off:off + 300 + q % 900])
        rows = o.query_sequences(qs)
        full = want_lists(o, rows, None, 3, 5.0)
        assert max(len(w) for w in full) > 64
        before = ix.stats()
        got, _ = ix.query_list(qs, None, 3, 5.0)
        assert ix.stats()["scan_slab_launches"] > before["scan_slab_launches"]
        assert_same(got, full)
        assert_same(ix.query_list(qs[:16], 70, 3, 5.0)[0], want_lists(o, rows[:16], 70, 3, 5.0))
        long_q = [seqs[7][:9000], seqs[8], seqs[G // 2][100:6000]]
        lrows = o.query_sequences(long_q)
        assert_same(ix.query_list(long_q, None, 3, 5.0)[0], want_lists(o, lrows, None, 3, 5.0))
    finally:
        ix.close()


def test_nan_corner_keeps_the_host_route(hip):
    """min_score 0 over an index with an empty sketch (a genome exactly k long, jaccard 0 / 0): not ordered on the device;
    the per-query host route answers, as mk_query's does (compared bit for bit: NaN is not equal to itself)"""
    import struct
    k, h = 21, 10
    seqs = [synth.genome_bases(70 + g, 0, 5000) for g in range(6)] + [synth.genome_bases(99, 0, k)]
    ix = hip.Miekki(k, h, 8, 32, 0)
    try:
        ix.insert_sequences(seqs)
        assert 0 in list(ix.sketch_size)
        qs = [seqs[0][:400], seqs[3][100:900]]
        bits = lambda res: [[(x.genome, x.matches, struct.pack("<dd", x.jaccard, x.intersection)) for x in r] for r in res]
        for N in (3, 7):
            assert bits(ix.query_list(qs, N, 0, 0.0)[0]) == bits(ix.query(qs, N, 0, 0.0)[0])
    finally:
        ix.close()


# ---- the binary: -n ------------------------------------------------------------------------------------------------------
CK, CH, CTHR, CSP, CST, CL = 31, 12, 100, 2, 80, 40_000


def run_cli(args, cwd, devices="0", ok=True):
    env = dict(os.environ, MIEKKI_DEVICES=devices)
    r = subprocess.run([CLI, *args], cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
    if ok:
        assert r.returncode == 0, r.stdout.decode(errors="replace")
    return r


@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    from oracle import oracle as orc
    d = tmp_path_factory.mktemp("strain_cli")
    G = CSP * CST
    seqs = [synth.strain_device(g, CST, PPM, 0, CL) for g in range(G)]
    names = [f"s{g}.fa" for g in range(G)]
    for fn, s in zip(names, seqs):
        (d / fn).write_bytes(synth.fasta(fn[:-3], s))
    (d / "genomes.lst").write_bytes(b"".join(fn.encode() + b"\n" for fn in names))
    whole = [names[g] for g in (0, 1, 85, 159)]
    (d / "qfiles.lst").write_bytes(b"".join(fn.encode() + b"\n" for fn in whole))
    qs = cut_queries(seqs, 120, 3) + [synth.genome_bases(5_000_000, 0, 1000)]
    heads = [f">q{i}".encode() for i in range(len(qs))]
    (d / "queries.fa").write_bytes(b"".join(h + b"\n" + s + b"\n" for h, s in zip(heads, qs)))
    o = orc.OracleMiekki(CK, CH, 8, 33, CTHR)
    o.insert_sequences(seqs)
    base = ["-k", str(CK), "-h", str(CH), "-s", str(CTHR), "-t", "1"]
    run_cli(["-l", "genomes.lst", "-d", "idx.gz", *base], d)
    return d, o, heads, o.query_sequences(qs), [w.encode() for w in whole], o.query_sequences([seqs[g] for g in (0, 1, 85, 159)])


def oracle_text(o, names, rows, N, skip_empty):
    n = o.index_size if N == 0 else N
    out = b""
    for name, row in zip(names, rows):
        hits = o.filter_results(row, n, 10, 0.5 * CTHR)
        if hits or not skip_empty:
            out += o.format_query_line(name, hits)
    return out


@pytest.mark.parametrize("N", [0, 100])
@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_cli_n_like_the_oracle(cli_dir, N, devices):
    """-a and -A with -n on the strain list, on one context and sharded over two contexts of GPU 0: same bytes"""
    d, o, heads, rows, whole, wrows = cli_dir
    assert max(len(o.filter_results(r, o.index_size, 10, 0.5 * CTHR)) for r in rows) > 64
    tag = f"{N}_{len(devices)}"
    run_cli(["-i", "idx.gz", "-a", "queries.fa", "-o", f"a{tag}.txt", "-n", str(N), "-t", "1"], d, devices)
    assert (d / f"a{tag}.txt").read_bytes() == oracle_text(o, heads, rows, N, False)
    run_cli(["-i", "idx.gz", "-A", "qfiles.lst", "-o", f"A{tag}.txt", "-n", str(N), "-t", "1"], d, devices)
    assert (d / f"A{tag}.txt").read_bytes() == oracle_text(o, whole, wrows, N, True)


def test_cli_default_is_n_10_and_exact_mode_refuses_n(cli_dir):
    d, o, heads, rows, _, _ = cli_dir
    a = run_cli(["-i", "idx.gz", "-a", "queries.fa", "-o", "d.txt", "-t", "1"], d).stdout
    b = run_cli(["-i", "idx.gz", "-a", "queries.fa", "-o", "d10.txt", "-n", "10", "-t", "1"], d).stdout
    assert (d / "d.txt").read_bytes() == (d / "d10.txt").read_bytes() == oracle_text(o, heads, rows, 10, False)
    assert a.replace(b"d.txt", b"X") .split(b"elapsed")[0] == b.replace(b"d10.txt", b"X").split(b"elapsed")[0]
    r = run_cli(["-i", "idx.gz", "-a", "queries.fa", "-o", "e.txt", "-n", "5", "-e", "-t", "1"], d, ok=False)
    assert r.returncode != 0 and b"-n" in r.stdout
    r = subprocess.run([CLI, "-i", "idx.gz", "-a", "queries.fa", "-o", "r.txt", "-n", "0"], cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120, env=dict(os.environ, MIEKKI_DEVICES="0", MIEKKI_WORLD="1", MIEKKI_RANK="0"))
    assert r.returncode != 0 and b"-n" in r.stdout              # one process per GPU: refused before any work
