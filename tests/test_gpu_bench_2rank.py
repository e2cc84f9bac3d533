"""bench.py --gpus 2 without a launcher: it must start two ranks itself (never report a 1-GPU run as n_gpus = 2) and, with
--full, run BASELINE configs[4]'s code — `rabitq_sharded` (row shards + one all-gather of per-shard top-k,
engine/search.go:835-908's fan-out/merge) and `pq_train_sharded` (sub-quantizer ranges, pq.go:83-138) — here with gloo, two
ranks sharing GPU 0 and reduced sizes (the line says so).  No scaling curve comes out of this: it proves the N > 1 code runs.
A plain run (no --full) times the headline and nothing else."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


# 4: 24 sub-quantizers per rank, a 4-list merge, four writers of one stdout.  The ranks share GPU 0 with this process and
# the launcher: a node's 8 would keep ten processes on one device at once, more than a shared GPU box admits.
@pytest.mark.parametrize("world", [2, 4])
def test_bench_gpus2_self_launch_gloo(world, tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VECGO_BENCH_ROWS="200000", VECGO_BENCH_SCAN_ROWS="200000")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", str(world), "--backend", "gloo", "--steps", "3", "--warmup", "1",
           "--full", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-3000:]   # nothing but the line (Gloo's own prints go to stderr)
    d = json.loads(lines[0])
    assert len(lines[0]) < 8192
    assert d["n_gpus"] == world and d["exchange"]["world_size"] == world and d["exchange"]["torch_backend"] == "gloo"
    assert d["reduced_sizes"] is True and "multi_gpu_legs_error" not in d
    assert d["recall_at_10"] == 1.0                   # the sharded exact path against the fp64 ground truth
    names = {c["config"]: c for c in d["configs"]}
    assert names["configs[4] rabitq sharded (strong)"]["qps"] > 0
    assert names["configs[4] rabitq sharded (weak)"]["rows_per_gpu"] == 200000
    assert names["configs[4] pq kmeans train, sharded by sub-quantizer"]["codebooks_identical_on_all_ranks"] is True
    rep = names["metric pipeline over query-sharded replicas (structured corpus)"]   # graph search = replicas
    assert rep["replicas"] == world and rep["ids_equal_single_gpu"] is True and rep["qps"] > 0 and rep["recall_at_10"] > 0.5
    assert "not measured" in d["scaling_curve"]
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    # rank 0's copy of the merged result of the last timed step: every query's 10 nearest rows, ascending distances
    ids, sc = np.load(tmp_path / "out" / "ids.npy"), np.load(tmp_path / "out" / "scores.npy")
    assert ids.shape == sc.shape == (1024, 10) and ids.dtype == np.float64 and sc.dtype == np.float32
    assert np.all((ids >= 0) & (ids < 200000)) and np.all(np.diff(sc, axis=1) >= 0)


def test_bench_plain_run_times_the_headline_only(tmp_path):
    """Without --full a run sets up, warms up, times its steps, dumps them and prints the line: the exact path with its recall
    against the fp64 ground truth and the roofline of the timed kernel, none of the extras (reduced sizes)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VECGO_BENCH_ROWS="200000", VECGO_BENCH_SCAN_ROWS="200000")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["config"]["operating_point"] == "flat_exact" and "--full" in d["config"]["operating_point_note"]
    assert d["recall_at_10"] == 1.0 and d["recall_queries"] == 1024
    assert d["roofline"]["bound"] == "mfma" and d["roofline"]["launches"] >= 3
    assert "cpu_baseline" not in d and [c["config"] for c in d["configs"]] == ["configs[1] flat exact fp32 MFMA GEMM"]
    ids, sc = np.load(tmp_path / "out" / "ids.npy"), np.load(tmp_path / "out" / "scores.npy")
    assert ids.shape == sc.shape == (1024, 10) and np.all((ids >= 0) & (ids < 200000)) and np.all(np.diff(sc, axis=1) >= 0)
