"""vg_search_flat_probed_threshold over SQ8 codes at 1M x 768 (the bench's rows), unpartitioned, 8 queries: GPU ms per call
  1. max_results 512, threshold +Inf, no rerank — next to vg_search_sq8(k = 512) on the same batch (pages of 64 results)
  2. max_results 16384 with rerank (the two-pass histogram form, then the exact re-score)
each with its stages (profile scopes probed_thr_scan / probed_thr_select / probed_thr_rerank), the bytes a pass over the codes
reads and the rate that implies.  Then the same over 122 IVF partitions, nprobes 8.  Usage: python tools/probed_threshold_time.py [rows]"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import vecgo_amd as vg, bench

ctx = vg.Context(0)
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dim = bench.DIM
rows = bench.gen_rows(0, n, dev)
q = bench.gen_queries(1, dev)[0][:8].contiguous()
idx = vg.Index(ctx, n, dim)
idx.set_vectors(rows)
sq = vg.ScalarQuantizer(ctx, dim)
sq.train(rows[:200000])
idx.set_sq8_codes(sq, sq.encode(rows))
st = torch.cuda.current_stream()
SCOPES = ("probed_thr_scan", "probed_thr_select", "probed_thr_rerank")


def timed(fn, reps=20):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stages(fn):
    for name in SCOPES:
        ctx.profile_read(name)
    ctx.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    ctx.profile_enable(False)
    return {name: ctx.profile_read(name) for name in SCOPES}


def report(label, nprobes, visible_rows):
    inf = torch.full((8,), float("inf"), device=dev)
    code_bytes = visible_rows * dim   # one pass over the codes a query can see (the whole segment: shared by the 8 queries)
    base = timed(lambda: idx.search_flat_probed(q, 512, nprobes, scan=idx.SCAN_SQ8, stream=st))
    for mr, rerank in ((512, False), (16384, True)):
        call = lambda: idx.search_flat_probed_threshold(q, inf, mr, nprobes, idx.SCAN_SQ8, rerank, stream=st)
        ms = timed(call)
        s = stages(call)
        scan_ms = s["probed_thr_scan"][1]
        passes = 2 if rerank else 1
        pass_bytes = code_bytes * (1 if nprobes == 0 else 8)
        print(f"{label} max_results={mr:5d} rerank={int(rerank)}: {ms:7.3f} ms per call  (scan {scan_ms:6.3f} ms = {passes} pass(es) of "
              f"{pass_bytes / 1e6:7.1f} MB of codes -> {passes * pass_bytes / scan_ms / 1e9:5.2f} TB/s; select {s['probed_thr_select'][1]:6.3f} ms, "
              f"rerank {s['probed_thr_rerank'][1]:6.3f} ms)   top-k scan k=512 (pages of 64): {base:7.3f} ms", flush=True)


report("whole segment, nq=8", 0, n)
parts = 122
cent = rows[torch.randperm(n, device=dev)[:parts]].contiguous()
assign = torch.cat([((rows[i:i + 65536] ** 2).sum(1)[:, None] - 2 * rows[i:i + 65536] @ cent.T + (cent ** 2).sum(1)[None, :]).argmin(1)
                    for i in range(0, n, 65536)])
order = torch.argsort(assign, stable=True)
off = torch.searchsorted(assign[order].contiguous(), torch.arange(parts + 1, device=dev)).to(torch.int32)
prow = rows[order].contiguous()
idx = vg.Index(ctx, n, dim)
idx.set_vectors(prow)
idx.set_sq8_codes(sq, sq.encode(prow))
idx.set_partitions(cent.cpu().numpy(), off.cpu().numpy().astype(np.uint32))
report(f"{parts} partitions, nprobes=8, nq=8", 8, int(8 * n / parts))
