"""vg_vamana_reorder_bfs wall time, warmed up, split into the BFS and the permutation (profile scopes vamana_reorder_bfs /
vamana_reorder_permute), with the BFS's level count and tail components and the permutation's HBM bytes (every array
read and written by the gather, then copied back out of the scratch buffer: 4 passes of its bytes).  Shapes:
  random   N x 768 fp32 rows (+ their norms), R 64, a random graph through set_vamana_graph (default N = 1M)
  built    200k x 128 rows, a vg_vamana_build graph (R 64, L 100)
  path     N nodes, node i lists i + 1: depth N
  empty    N nodes, every list empty: N singleton components
Prints one JSON line.  Usage: python tools/vamana_reorder_time.py [rows]"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import vecgo_amd as vg
from tests import reorder_bfs_ref as ref

ctx = vg.Context(0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
X = ref.INVALID
rng = np.random.default_rng(1)
out = {"rows": n}


def timed(idx, g, entry, reps=3):
    for s in ("vamana_reorder_bfs", "vamana_reorder_permute"):
        ctx.profile_read(s)
    idx.set_vamana_graph(g, entry)
    idx.reorder_vamana_bfs()  # warm-up (scratch, code objects)
    wall, bfs, perm = [], [], []
    ctx.profile_enable(True)
    for _ in range(reps):
        idx.set_vamana_graph(g, entry)  # the same permutation again (of the already permuted rows: same traffic)
        ctx.profile_read("vamana_reorder_bfs"), ctx.profile_read("vamana_reorder_permute")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.reorder_vamana_bfs()
        wall.append((time.perf_counter() - t0) * 1e3)
        bfs.append(ctx.profile_read("vamana_reorder_bfs")[1])
        perm.append(ctx.profile_read("vamana_reorder_permute")[1])
    ctx.profile_enable(False)
    return {"wall_ms": round(min(wall), 2), "bfs_ms": round(min(bfs), 2), "permute_ms": round(min(perm), 2)}


def random_graph(rows, r):
    return rng.integers(0, rows, (rows, r), dtype=np.int64).astype(np.uint32)


# random: N x 768, R 64
dim, r = 768, 64
g = random_graph(n, r)
idx = vg.Index(ctx, n, dim)
idx.set_vectors(rng.standard_normal((n, dim), dtype=np.float32))
st = {}
ref.reorder_np(g, n // 2, st)
res = timed(idx, g, n // 2)
moved = 4 * (n * dim * 4 + n * 4 + n * r * 4)
res.update(levels=st["levels"], tails=st["tails"], permute_gb=round(moved / 1e9, 2),
           permute_gbps=round(moved / 1e9 / (res["permute_ms"] / 1e3), 0))
out["random_768_r64"] = res
del idx

# built: 200k x 128, vg_vamana_build R 64
bn, bdim = 200_000, 128
idx = vg.Index(ctx, bn, bdim)
idx.set_vectors(rng.standard_normal((bn, bdim), dtype=np.float32))
t0 = time.perf_counter()
idx.build_vamana(r=64, l=100)
build_s = time.perf_counter() - t0
bg, be = idx.get_vamana_graph()
st = {}
ref.reorder_np(bg, be, st)
res = timed(idx, bg, be)
res.update(levels=st["levels"], tails=st["tails"], build_s=round(build_s, 1))
out["built_200k_128_r64"] = res
del idx

# degenerate shapes, graph only
for shape in ("path", "empty"):
    g = np.full((n, 64), X, np.uint32)
    if shape == "path":
        g[:-1, 0] = np.arange(1, n)
    idx = vg.Index(ctx, n, 4)
    res = timed(idx, g, 0, reps=1)
    res.update(levels=n, tails=0 if shape == "path" else n - 1)
    out[shape + "_r64"] = res
    del idx
print(json.dumps(out))
