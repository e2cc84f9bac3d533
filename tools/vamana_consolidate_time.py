"""vg_vamana_consolidate on a resident Vamana graph: N0 x DIM uniform rows are built into a graph by vg_vamana_build and INS
more rows inserted by vg_vamana_insert (tools/vamana_insert_time.py's graph, default options: R 64, L 100, alpha 1.2), then a
share DEL of the rows is deleted at random (0.1 = the reference's trigger) and one vg_vamana_consolidate at max_batch 8192 is
timed: the graph is put back before every run, one warm-up run, RUNS timed runs (host clock around the call, which ends in a
stream synchronise): median, min and max seconds, us per repaired node, the counters; the stage split (mark / search /
prune, profiler events) from a run of its own.  Beside it the yardsticks: vg_vamana_build over the live rows only, and
the insert's us per node from this process; recall@10 of vg_search_vamana_fresh over the live rows before the consolidate,
after it, and over the rebuilt graph; graph_crc32: zlib.crc32 over the bytes and entry point of the graph before the consolidate,
after it, and rebuilt (two libraries that compute the same thing print the same).  One JSON line.
usage: vamana_consolidate_time.py [N0 INS DIM DEL RUNS]   (default 80000 20000 128 0.1 5)"""
import sys, time, json, statistics, zlib
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import vecgo_amd as vg

STAGES = {"mark": "vamana_consolidate_mark", "search": "vamana_consolidate_search", "prune": "vamana_consolidate_prune"}
args = sys.argv[1:6] + ["80000", "20000", "128", "0.1", "5"][len(sys.argv) - 1:]
n0, ins, dim, share, runs = int(args[0]), int(args[1]), int(args[2]), float(args[3]), int(args[4])
n = n0 + ins
ctx = vg.Context(0); dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev); gen.manual_seed(0)
rows = torch.rand((n, dim), generator=gen, device=dev, dtype=torch.float32)
deleted = np.random.default_rng(0).random(n) < share
live = np.nonzero(~deleted)[0]
packed = np.packbits(deleted, bitorder="little")  # what a host keeps: one bit per node
live_rows = rows[torch.from_numpy(live).to(dev)].contiguous()
queries = live_rows[torch.randperm(live.size, generator=gen, device=dev)[:256]].contiguous()
truth = live[torch.cdist(queries, live_rows).topk(10, largest=False).indices.cpu().numpy()]  # exact, over the live rows
queries = queries.cpu().numpy()


def recall(idx, dele, ids_of=None):
    ids, _, _ = idx.search_vamana_fresh(queries, 10, deleted=dele)
    if ids_of is not None:
        ids = np.where(ids == 0xFFFFFFFF, ids, ids_of[np.minimum(ids, ids_of.size - 1)])
    return round(float((ids[:, :, None] == truth[:, None, :]).any(2).mean()), 4)


def crc(idx):
    g, e = idx.get_vamana_graph()
    return zlib.crc32(int(e).to_bytes(4, "little"), zlib.crc32(g.tobytes()))


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


idx = vg.Index(ctx, n0, dim); idx.set_vectors(rows[:n0])
build0_s, _ = wall(lambda: idx.build_vamana())
insert_s, _ = wall(lambda: idx.insert_vamana(rows[n0:]))
g0, entry = idx.get_vamana_graph()
recall_before = recall(idx, deleted)
crcs = {"before": crc(idx)}

times, stats = [], None
for run in range(runs + 1):  # the first one warms up
    idx.set_vamana_graph(g0, entry)
    s, stats = wall(lambda: idx.consolidate_vamana(packed))
    if run:
        times.append(s)
recall_after = recall(idx, deleted)
crcs["after"] = crc(idx)
assert idx.consolidate_vamana(packed)["repaired_nodes"] == 0  # idempotent
idx.set_vamana_graph(g0, entry)
ctx.profile_enable(True)
idx.consolidate_vamana(packed)
torch.cuda.synchronize()
stage_ms = {k: round(ctx.profile_read(v)[1], 2) for k, v in STAGES.items()}
ctx.profile_enable(False)
idx.close()

rebuilt = vg.Index(ctx, live.size, dim); rebuilt.set_vectors(live_rows)
rebuild_s, _ = wall(lambda: rebuilt.build_vamana())
crcs["rebuilt"] = crc(rebuilt)
med = statistics.median(times)
print(json.dumps({
    "n": n, "dim": dim, "deleted": int(deleted.sum()), "max_batch": 8192, "runs": runs, "stats": stats,
    "consolidate_s": {"median": round(med, 4), "min": round(min(times), 4), "max": round(max(times), 4)},
    "consolidate_us_per_repaired_node": round(med / max(stats["repaired_nodes"], 1) * 1e6, 2),
    "consolidate_stages_ms": stage_ms,
    "insert_us_per_node": round(insert_s / ins * 1e6, 2), "build_n0_us_per_node": round(build0_s / n0 * 1e6, 2),
    "rebuild_live_s": round(rebuild_s, 3), "rebuild_live_us_per_node": round(rebuild_s / live.size * 1e6, 2),
    "graph_crc32": crcs,
    "recall10": {"before": recall_before, "after": recall_after, "rebuilt": recall(rebuilt, None, ids_of=live)}}), flush=True)
