"""vg_hnsw_insert into a resident HNSW graph of N x 768 i.i.d. normal rows (M = 32, EF = 300): the graph is built with
vg_hnsw_build over the first N rows, then inserts of 1, 64, 1024 and 8192 rows follow one another; per call the wall ms
and the stage split (search / select / state derivation / back links, profiler events).  One JSON line per N.
usage: hnsw_insert_time.py [N ...]   (default 100000 1000000)"""
import sys, time, json
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench

SIZES = (1, 64, 1024, 8192)
STAGES = {"search": "hnsw_build_search", "select": "hnsw_build_select", "derive": "hnsw_insert_derive",
          "link": "hnsw_build_link"}
D = 768
ctx = vg.Context(0); dev = torch.device("cuda", 0)
for n in [int(x) for x in sys.argv[1:]] or [100_000, 1_000_000]:
    rows = bench.gen_rows(0, n + sum(SIZES), dev)
    idx = vg.Index(ctx, n, D); idx.set_vectors(rows[:n])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    idx.build_hnsw(m=32, ef_construction=300)
    torch.cuda.synchronize(); build_s = time.perf_counter() - t0
    out, at = {"n": n, "build_s": round(build_s, 3), "inserts": []}, n
    for c in SIZES:
        ctx.profile_enable(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        idx.insert_hnsw(rows[at:at + c], m=32, ef_construction=300)
        torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
        st = {k: round(ctx.profile_read(v)[1], 3) for k, v in STAGES.items()}
        ctx.profile_enable(False)
        out["inserts"].append({"rows": c, "into": at, "ms": round(ms, 3), "stages_ms": st})
        at += c
    print(json.dumps(out), flush=True)
    idx.close(); del rows
