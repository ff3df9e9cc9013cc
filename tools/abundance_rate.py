"""What does the abundance estimate cost: the collect pass beside the tally's walk, a round over the pool, and 50 rounds end to
end beside the only route there was before?  (recorded, not gated: profiles/abundance.txt)

The inputs of profiles/read_lca.txt -- 20,000 synthetic strain genomes in families of 64 at -h 17, 20,000 reads of 1 kb cut
from genomes drawn at random, as ONE uploaded set that is invalidated before every pass, so that a pass is complete (sketch,
Bloom gate, scan, walk) -- with the families as runs of ids (grouped, what -K <families file> leaves) and with the ids permuted
at random (ungrouped), at margins 100 and 10.  Per case, one warm-up and --repeats timed runs, medians:
  (t)  mk_qset_run_tally                        filter_ms: one walk per read
  (c)  mk_qset_run_share                        filter_ms: two or three walks per shared read, the scan, one read of two totals
  (r)  one round over the pool                  (filter_ms of 201 rounds - filter_ms of 1 round) / 200, per MIEKKI_SHARE_TEAM
  (e)  collect + mk_share_rounds, R = 50        wall clock, scan included
  (h)  mk_qset_run_list(MK_LIST_CANDIDATES),    wall clock: the only route to this answer before -- every hit of every read to
       the margin rule and 50 rounds in numpy   the host, tests/share_ref.py's rule vectorised in 64-bit integers
The host route's abundances, delta and starved count must equal the device's before anything is reported.  20,000 reads fill a
pool that a round crosses in the time of its two launches, so (r) is also taken over hand-made pools of 4 M reads of 2 ids, 2 M of
4, 1 M of 16 and 250 k of 64 (mk_share_add_lists; runs of ids inside a family): there the mapping of reads to lanes shows.

    python tools/abundance_rate.py [--genomes 20000] [--queries 20000] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HIT = np.dtype([("genome", "<u4"), ("matches", "<u4"), ("jaccard", "<f8"), ("intersection", "<f8")])
AUTO = 0xffffffff


def host_pool(off, rec, margin, G):
    """the header's rule over the lists of all reads, in numpy: (unique [G], ids of the shared reads, their starts, N)"""
    off = np.asarray(off, np.int64)
    n = np.diff(off)
    seg = np.repeat(np.arange(len(n)), n)
    g, x = rec["genome"].astype(np.int64), rec["intersection"]
    has = np.flatnonzero(n > 0)
    best = np.zeros(len(n))
    best[has] = np.maximum.reduceat(x, off[has])
    keep = x * 100.0 >= best[seg] * float(100 - margin)
    g, seg = g[keep], seg[keep]
    size = np.bincount(seg, minlength=len(n))
    unique = np.bincount(g[size[seg] == 1], minlength=G).astype(np.uint64)
    several = size[seg] >= 2
    ids = g[several]
    lens = size[size >= 2]
    starts = np.r_[0, np.cumsum(lens)[:-1]].astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    return unique, ids, starts, lens.astype(np.uint64), int((size >= 1).sum())


def host_rounds(unique, ids, starts, lens, N, R, G):
    """the rounds in 64-bit integers: (A_R, delta, starved)"""
    s = np.uint64(int(N).bit_length())
    order = np.argsort(ids, kind="stable")
    by_g = ids[order]
    g_start = np.flatnonzero(np.r_[True, by_g[1:] != by_g[:-1]]) if len(ids) else np.zeros(0, np.int64)
    g_of = by_g[g_start] if len(ids) else np.zeros(0, np.int64)
    seg = np.repeat(np.arange(len(lens)), lens.astype(np.int64))
    p = np.ones(G, np.uint64)
    before = np.zeros(G, np.uint64)
    starved = 0
    for _ in range(R):
        A = unique << np.uint64(32)
        if len(ids):
            w = p[ids]
            D = np.add.reduceat(w, starts)
            dry = D == 0
            starved = int(dry.sum())
            share = np.where(dry[seg], np.uint64(1 << 32) // lens[seg], (w << np.uint64(32)) // np.where(dry, np.uint64(1), D)[seg])
            A[g_of] += np.add.reduceat(share[order], g_start)
        delta = int(np.where(A > before, A - before, before - A).sum())
        before = A
        p = A >> s
    return before, delta, starved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=20_000)
    ap.add_argument("--queries", type=int, default=20_000)
    ap.add_argument("--length", type=int, default=200_000)
    ap.add_argument("--strains", type=int, default=64)
    ap.add_argument("--rate-ppm", type=int, default=3000)
    ap.add_argument("--h", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import miekki_amd
    import synth
    from miekki_amd import lib as L
    lib = L.load_library()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, NQ, thr = args.genomes, args.queries, 200
    mi = 0.5 * thr
    ix = miekki_amd.Miekki(31, args.h, 8, 33, thr)
    ix.reserve(G)
    for g0 in range(0, G, 2048):
        ix.insert_synthetic_strains(g0, min(2048, G - g0), args.length, args.strains, args.rate_ppm)
    L.check(lib.mk_sync(ix._h))
    gbps, nbytes = C.c_double(0), C.c_uint64(0)
    L.check(lib.mk_probe_stream_read(ix._h, 3, C.byref(gbps), C.byref(nbytes)))
    say(f"index: {G} strain genomes x {args.length} bases, families of {args.strains}, {args.rate_ppm} ppm, -k 31 -h {args.h}; "
        f"{NQ} reads of 1 kb from genomes at random, thresholds (10, {mi}); {args.repeats} timed runs after one warm-up, medians; "
        f"stream probe {gbps.value:.0f} GB/s")
    rng = np.random.default_rng(8)
    reads = [synth.strain_device(int(rng.integers(0, G)), args.strains, args.rate_ppm, int(rng.integers(0, args.length - 1000)), 1000) for _ in range(NQ)]
    ptrs, lens = L.seq_arrays(reads)
    d_tally = C.c_void_p()
    L.check(lib.mk_dev_alloc(ix._h, 32 * G, C.byref(d_tally)))

    def med(f, n=args.repeats):
        f()
        return float(np.median([f() for _ in range(n)]))

    def layout(name):
        qs = C.c_void_p()
        L.check(lib.mk_qset_upload(ix._h, ptrs, lens, NQ, C.byref(qs)))

        def tally_pass():
            ix.reset_stats()
            L.check(lib.mk_qset_invalidate(ix._h, qs))
            L.check(lib.mk_tally_reset(ix._h, d_tally, G))
            L.check(lib.mk_qset_run_tally(ix._h, qs, 10, mi, d_tally, G))
            out = np.zeros((G, 4), np.uint64)
            L.check(lib.mk_tally_read(ix._h, d_tally, G, out.ctypes.data))
            tally_pass.out = out
            return ix.stats()["filter_ms"]

        t_ms = med(tally_pass)
        adds = int(tally_pass.out[:, 0].sum()) + 3 * int(tally_pass.out[:, 2].sum())
        say(f"{name}: (t) tally walk filter_ms {t_ms:.3f}: {adds} adds, {adds / t_ms / 1e6:.2f} G adds/s")
        for margin in (100, 10):
            pool = C.c_void_p()
            L.check(lib.mk_share_create(ix._h, C.byref(pool)))
            info, res, a = L.ShareInfo(), L.ShareResult(), np.zeros(G, np.uint64)

            def collect():
                ix.reset_stats()
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                L.check(lib.mk_share_reset(ix._h, pool))
                L.check(lib.mk_qset_run_share(ix._h, qs, 10, mi, margin, pool))
                return ix.stats()["filter_ms"]

            c_ms = med(collect)
            L.check(lib.mk_share_info_read(ix._h, pool, C.byref(info)))
            n_reads, n_ids = int(info.shared_reads), int(info.entries)
            say(f"  margin {margin}: {int(info.assigned)} assigned, {n_reads} shared, {n_ids} ids stored "
                f"({n_ids / max(n_reads, 1):.1f} per shared read); (c) collect filter_ms {c_ms:.3f} = {c_ms / t_ms:.2f} x (t)")

            def rounds_ms(R):
                ix.reset_stats()
                L.check(lib.mk_share_rounds(ix._h, pool, R, AUTO, a.ctypes.data, C.byref(res)))
                return ix.stats()["filter_ms"]

            pool_bytes = 4 * n_ids + 8 * (n_reads + 1)
            for team in ("16", "8", "32", "64"):
                os.environ["MIEKKI_SHARE_TEAM"] = team
                per = (med(lambda: rounds_ms(201)) - med(lambda: rounds_ms(1))) / 200
                say(f"    (r) team {team:>2}: {per * 1e3:8.1f} us per round, {n_ids / max(per, 1e-9) / 1e6:6.2f} G ids/s, "
                    f"pool read at {pool_bytes / max(per, 1e-9) / 1e6:6.1f} GB/s")
            del os.environ["MIEKKI_SHARE_TEAM"]

            def device_route():
                t0 = time.perf_counter()
                collect()
                L.check(lib.mk_share_rounds(ix._h, pool, 50, AUTO, a.ctypes.data, C.byref(res)))
                return (time.perf_counter() - t0) * 1e3

            e_ms = med(device_route)
            got = (a.copy(), int(res.delta), int(res.starved))

            def host_route():
                t0 = time.perf_counter()
                L.check(lib.mk_qset_invalidate(ix._h, qs))
                hl = C.c_void_p()
                L.check(lib.mk_qset_run_list(ix._h, qs, L.LIST_CANDIDATES, 10, mi, C.byref(hl)))
                off = np.ctypeslib.as_array(lib.mk_hitlist_offsets(hl), (NQ + 1,)).copy()
                rec = np.zeros(int(off[NQ]), HIT)
                if len(rec):
                    C.memmove(rec.ctypes.data, lib.mk_hitlist_hits(hl), rec.nbytes)
                lib.mk_hitlist_free(hl)
                t1 = time.perf_counter()
                host_route.out = host_rounds(*host_pool(off, rec, margin, G), 50, G)
                host_route.lists_ms = (t1 - t0) * 1e3
                return (time.perf_counter() - t0) * 1e3

            h_ms = med(host_route, 1)
            want = host_route.out
            if not (np.array_equal(got[0], want[0]) and got[1:] == want[1:]):
                raise SystemExit(f"{name}, margin {margin}: the host route and the device disagree")
            say(f"    (e) collect + 50 rounds, wall {e_ms:.1f} ms; (h) lists to the host + numpy, wall {h_ms:.1f} ms "
                f"({host_route.lists_ms:.1f} ms of it the lists): {h_ms / e_ms:.2f} x; the two agree bit for bit, last change {got[1] / 2 ** 32:.3f} reads, "
                f"{got[2]} starved")
            lib.mk_share_free(ix._h, pool)
        lib.mk_qset_free(ix._h, qs)

    def large_pools():
        """pools that no 20,000 reads fill, through mk_share_add_lists: runs of ids inside a family, and 20,000 settled reads"""
        r = np.random.default_rng(5)
        singles = r.integers(0, G, 20_000).astype(np.uint32)
        for n, length in ((4_000_000, 2), (2_000_000, 4), (1_000_000, 16), (250_000, 64)):
            first = (r.integers(0, G // args.strains, n) * args.strains + r.integers(0, args.strains - length + 1, n)).astype(np.uint32)
            ids = np.concatenate([(first[:, None] + np.arange(length, dtype=np.uint32)[None, :]).ravel(), singles])
            off = np.concatenate([np.arange(n, dtype=np.uint64) * np.uint64(length), np.uint64(n * length) + np.arange(len(singles) + 1, dtype=np.uint64)])
            pool = C.c_void_p()
            L.check(lib.mk_share_create(ix._h, C.byref(pool)))
            L.check(lib.mk_share_add_lists(ix._h, pool, off.ctypes.data, ids.ctypes.data, len(off) - 1))
            res, a = L.ShareResult(), np.zeros(G, np.uint64)

            def rounds_ms(R):
                ix.reset_stats()
                L.check(lib.mk_share_rounds(ix._h, pool, R, AUTO, a.ctypes.data, C.byref(res)))
                return ix.stats()["filter_ms"]

            n_ids, pool_bytes = n * length, 4 * n * length + 8 * (n + 1)
            say(f"hand-made pool, {n} reads of {length} ids in runs, {n_ids} ids, {len(singles)} settled reads:")
            for team in ("16", "8", "32", "64"):
                os.environ["MIEKKI_SHARE_TEAM"] = team
                per = (med(lambda: rounds_ms(21)) - med(lambda: rounds_ms(1))) / 20
                say(f"    (r) team {team:>2}: {per * 1e3:8.1f} us per round, {n_ids / max(per, 1e-9) / 1e6:6.2f} G ids/s, "
                    f"pool read at {pool_bytes / max(per, 1e-9) / 1e6:6.1f} GB/s")
            del os.environ["MIEKKI_SHARE_TEAM"]
            lib.mk_share_free(ix._h, pool)

    layout("grouped ids")
    large_pools()
    ix.select(np.random.default_rng(3).permutation(G).astype(np.uint32))
    layout("ungrouped ids")
    lib.mk_dev_free(ix._h, d_tally)
    ix.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
