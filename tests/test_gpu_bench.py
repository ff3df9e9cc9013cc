"""bench.py on the GPU box: the one-GPU line at a small size and the 2-rank rehearsal of the
default (strong-scaling) multi-GPU workload -- gloo collectives, both ranks on GPU 0, started
from a cold shell the way the driver starts it (plain `python bench.py --gpus 2 ...`)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, *argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1                                       # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_one_gpu_line_and_two_rank_rehearsal_agree():
    common = ["--genomes", "192", "--queries", "2000", "--h", "20", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"]
    one = run_bench("--gpus", "1", *common)
    two = run_bench("--gpus", "2", "--rehearse", *common)
    for r, n in ((one, 1), (two, 2)):
        assert r["n_gpus"] == n and r["scaling"] == "strong" and r["config"]["genomes_total"] == 192
        assert r["unit"] == "comparisons/s" and r["value"] > 0
        assert r["roofline"]["frac"] == pytest.approx(r["roofline"]["achieved"] / r["roofline"]["peak"])
        assert r["roofline"]["hbm_floor_bytes"] == (1 << 20) * r["config"]["genomes_per_gpu"]
        assert r["merge"]["overflowed_queries"] == 0
        # every query comes out with its source genome on top, and the device heap is the host heap
        assert r["check"]["top_hit_is_source_genome_of_all_queries"] == r["check"]["queries"] == 2000
        assert r["check"]["device_heap_equals_host_heap_of_strided_sample"] == r["check"]["strided_sample"] == 2000
    assert two["config"]["genomes_per_gpu"] == 96
    # same problem, same gate: identical active partitions, hence identical comparisons per step
    assert one["config"]["active_partitions_per_query"] == two["config"]["active_partitions_per_query"]
    assert two["merge"]["gather_bytes_per_rank"] == 2000 * (two["merge"]["cap"] + 1) * 8
    assert one["merge"]["gather_bytes_per_rank"] == 0


def test_plain_line_is_the_headline_and_dumps_the_last_steps_hits(tmp_path):
    """A plain run prints the headline without the --full extras and, with --dump-outputs, writes the last timed step's
    hits as float64 arrays: every query's top hit is its source genome (query q was cut from genome q mod G)."""
    import numpy as np
    G, Q = 192, 2000
    r = run_bench("--gpus", "1", "--genomes", str(G), "--queries", str(Q), "--h", "20", "--steps", "2", "--warmup", "1",
                  "--dump-outputs", str(tmp_path / "out"))
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["value"] > 0 and r["unit"] == "comparisons/s"
    assert r["higher_is_better"] is True and r["dtype"] == "u8" and r["merge"]["overflowed_queries"] == 0
    assert not {"roofline", "check", "cpu_baseline"} & set(r) and "roofline" not in r["sketch"]
    files = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(files) == {"query.npy", "nhits.npy", "hits_genome.npy", "hits_matches.npy", "hits_jaccard.npy",
                          "hits_intersection.npy"}
    assert all(a.dtype == np.float64 for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64_000_000
    assert np.array_equal(files["query.npy"], np.arange(Q))
    nh = files["nhits.npy"]
    assert nh.shape == (Q,) and ((nh >= 1) & (nh <= 10)).all()
    assert np.array_equal(files["hits_genome.npy"][:, 0], np.arange(Q) % G)
    assert (files["hits_matches.npy"][:, 0] >= 10).all() and (files["hits_jaccard.npy"][:, 0] > 0).all()
