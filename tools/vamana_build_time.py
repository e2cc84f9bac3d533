"""vg_vamana_build at N x 768 (the bench's rows; default 1M) with NewWriter's defaults (R 64, L 100, alpha 1.2,
max_batch 8192): wall seconds, the stage times (profile scopes vamana_build_search / _prune / _backedge), graph degree,
then recall@10 and QPS of vg_search_vamana kinds 0 (fp32 rows) and 1 (PQ codes, m 96) over 1024 queries on the built
graph against the HNSW layer-0 stand-in graph the bench walks.  Prints one JSON line.
Usage: python tools/vamana_build_time.py [rows]"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import vecgo_amd as vg, bench

ctx = vg.Context(0)
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rows = bench.gen_rows(0, n, dev)
q = bench.gen_queries(1, dev)[0]
st = torch.cuda.current_stream()
idx = vg.Index(ctx, n, bench.DIM)
idx.set_vectors(rows)
truth, _ = idx.search_flat(q, 10)
truth = truth.cpu().numpy() if hasattr(truth, "cpu") else truth
out = {"rows": n, "dim": bench.DIM, "r": 64, "l": 100, "alpha": 1.2, "max_batch": 8192}

stages = ("vamana_build_search", "vamana_build_prune", "vamana_build_backedge")
for s in stages:
    ctx.profile_read(s)
ctx.profile_enable(True)
torch.cuda.synchronize()
t0 = time.time()
idx.build_vamana(r=64, l=100, alpha=1.2, max_batch=8192)
torch.cuda.synchronize()
out["build_s"] = round(time.time() - t0, 3)
for s in stages:
    launches, ms = ctx.profile_read(s)
    out[s + "_ms"] = round(ms, 1)
ctx.profile_enable(False)
vgraph, ventry = idx.get_vamana_graph()
deg = (vgraph != 0xFFFFFFFF).sum(1)
out["degree_mean"], out["degree_min"] = round(float(deg.mean()), 2), int(deg.min())
print(json.dumps(out), flush=True)

pq = vg.ProductQuantizer(ctx, bench.DIM, 96, 256)
pq.train(rows[:20000], iters=4, seed=7, stream=st)
idx.set_pq_codes(pq, pq.encode(rows, stream=st))
t0 = time.time()
idx.build_hnsw(m=32, ef_construction=300)
torch.cuda.synchronize()
out["hnsw_build_s"] = round(time.time() - t0, 3)
l0, _, hentry = idx.get_hnsw_graph()


def recall(ids):
    ids = ids.cpu().numpy() if hasattr(ids, "cpu") else ids
    return round(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / 10 for a, b in zip(ids, truth)])), 4)


for name, graph, entry in (("vamana_built", vgraph, ventry), ("hnsw_layer0", l0, hentry)):
    idx.set_vamana_graph(graph, entry)
    for kind in (0, 1):
        ids, _ = idx.search_vamana(q, 10, kind=kind)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(3):
            idx.search_vamana(q, 10, kind=kind)
        torch.cuda.synchronize()
        dt = (time.time() - t0) / 3
        out[f"{name}_kind{kind}_recall10"] = recall(ids)
        out[f"{name}_kind{kind}_qps"] = round(q.shape[0] / dt, 1)
print(json.dumps(out), flush=True)
