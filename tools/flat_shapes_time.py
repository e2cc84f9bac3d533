"""vg_search_flat (fp32, 1M x 768) at the shapes beside the benchmark's that a change to the nomination must not slow down: one
call of 4096 queries (four 256-query tiles per workgroup of the persistent tile), k = 48 at 1024 queries (the split tile without
its screen), 129 queries (one ragged 256-query tile) and the benchmark's own 1024 x k = 10 — ms per call from stream events, and
what flat_stats / flat_retried / flat_appended counted per query.  The same command on two builds compares them.
    python tools/flat_shapes_time.py [repeats]"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench
ctx = vg.Context(0); dev = torch.device("cuda", 0)
rows = bench.gen_rows(0, 1_000_000, dev)
g = torch.Generator(device="cuda"); g.manual_seed(7)
q = torch.cat([bench.gen_queries(1, dev)[0], torch.randn(4096 - bench.Q_BATCH, 768, device="cuda", generator=g)])  # the benchmark's first
idx = vg.Index(ctx, 1_000_000, 768); idx.set_vectors(rows)
st = torch.cuda.current_stream()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2
appended = getattr(idx, "flat_appended", lambda: 0)   # (a build from before the counter: 0)
for nq, k, calls in ((1024, 10, 10), (4096, 10, 4), (1024, 48, 10), (129, 10, 10)):
    qs = q[:nq].contiguous()
    for _ in range(2): idx.search_flat(qs, k, stream=st)
    torch.cuda.synchronize()
    for rep in range(reps):
        s0, r0, a0 = idx.flat_stats(), idx.flat_retried(), appended()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls): idx.search_flat(qs, k, stream=st)
        e1.record(st); torch.cuda.synchronize()
        s1, r1, a1 = idx.flat_stats(), idx.flat_retried(), appended()
        per = calls * nq
        print(f"{nq:5d} queries k = {k:2d}: {e0.elapsed_time(e1) / calls:7.3f} ms per call   exhaustive {(s1[1] - s0[1]) / per:.4f}  "
              f"retried {(r1 - r0) / per:.4f}  appended {(a1 - a0) / per:.1f} per query", flush=True)
