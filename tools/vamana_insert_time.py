"""vg_vamana_insert into a resident Vamana graph: N0 x DIM uniform rows are built into a graph by vg_vamana_build, then
INS more rows are inserted in one call with default options (R 64, L 100, alpha 1.2) and the build's default batching
(max_batch 8192, growth_div 32); wall seconds, us per inserted node and the stage split (search / prune / reverse edges,
profiler events).  Beside it the yardstick: vg_vamana_build over all N0 + INS rows, us per node (two passes per node),
and recall@10 of vg_search_vamana_fresh over either graph; graph_crc32: zlib.crc32 over either graph's bytes and entry point
(two libraries that compute the same thing print the same).  One JSON line.
usage: vamana_insert_time.py [N0 INS DIM]   (default 80000 20000 128)"""
import sys, time, json, zlib
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg

STAGES = {"search": "vamana_insert_search", "prune": "vamana_insert_prune", "reverse": "vamana_insert_reverse"}
BUILD_STAGES = {"search": "vamana_build_search", "prune": "vamana_build_prune", "backedge": "vamana_build_backedge"}
n0, ins, dim = ([int(x) for x in sys.argv[1:4]] + [80_000, 20_000, 128][len(sys.argv) - 1:])[:3]
n = n0 + ins
ctx = vg.Context(0); dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev); gen.manual_seed(0)
rows = torch.rand((n, dim), generator=gen, device=dev, dtype=torch.float32)
queries = rows[torch.randperm(n, generator=gen, device=dev)[:256]].contiguous()
truth = torch.cdist(queries, rows).topk(10, largest=False).indices.cpu().numpy()
queries = queries.cpu().numpy()


def recall(idx):
    ids, _, _ = idx.search_vamana_fresh(queries, 10)
    return round(float((ids[:, :, None] == truth[:, None, :]).any(2).mean()), 4)


def crc(idx):
    g, entry = idx.get_vamana_graph()
    return zlib.crc32(int(entry).to_bytes(4, "little"), zlib.crc32(g.tobytes()))


def timed(fn, stages):
    ctx.profile_enable(True)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(); s = time.perf_counter() - t0
    st = {k: round(ctx.profile_read(v)[1], 1) for k, v in stages.items()}
    ctx.profile_enable(False)
    return s, st


idx = vg.Index(ctx, n0, dim); idx.set_vectors(rows[:n0])
b0_s, _ = timed(lambda: idx.build_vamana(), BUILD_STAGES)
ins_s, ins_st = timed(lambda: idx.insert_vamana(rows[n0:]), STAGES)
out = {"n0": n0, "inserted": ins, "dim": dim, "build_n0_s": round(b0_s, 3), "insert_s": round(ins_s, 3),
       "insert_us_per_node": round(ins_s / ins * 1e6, 1), "insert_stages_ms": ins_st, "recall10_after_insert": recall(idx),
       "graph_crc32": {"after_insert": crc(idx)}}
idx.close()
full = vg.Index(ctx, n, dim); full.set_vectors(rows)
b_s, b_st = timed(lambda: full.build_vamana(), BUILD_STAGES)
out.update({"build_n_s": round(b_s, 3), "build_us_per_node": round(b_s / n * 1e6, 1), "build_stages_ms": b_st,
            "recall10_built": recall(full)})
out["graph_crc32"]["built"] = crc(full)
print(json.dumps(out), flush=True)
