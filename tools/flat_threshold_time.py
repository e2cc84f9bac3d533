"""vg_search_flat_threshold (Engine.SearchThreshold's flat-segment leg) at 1M x 768 (the bench's rows): GPU ms per call for
1 / 4 / 64 / 1024 queries, thresholds at ranks 10 / 100 / 1000 / 10000 / 100000 of each query, max_results 100 / 16384, with and without the
bf16 filter — next to vg_search_flat at k = min(rank, 512) on the same batch.  Also each stage's share (profile
scopes flat_thr_gemm / flat_thr_rescore / flat_thr_scan / flat_thr_select) and the proof fall-backs.  Usage: python tools/flat_threshold_time.py [rows]"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench

ctx = vg.Context(0)
dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rows = bench.gen_rows(0, n, dev)
qall = bench.gen_queries(1, dev)[0]
idx = vg.Index(ctx, n, 768)
idx.set_vectors(rows)
st = torch.cuda.current_stream()
# thresholds at a rank of every query: the rank-th smallest fp32 squared distance (|x|^2 - 2 q.x + |q|^2)
rn = (rows * rows).sum(1)
thr = {}
for rank in (10, 100, 1000, 10000, 100000):
    parts = []
    for q0 in range(0, qall.shape[0], 64):
        qq = qall[q0:q0 + 64]
        s = rn[None, :] - 2 * qq @ rows.T + (qq * qq).sum(1)[:, None]
        parts.append(s.kthvalue(rank, dim=1).values)
    thr[rank] = torch.cat(parts).contiguous()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for mode in ("fp32", "bf16 filter"):
    idx.enable_bf16_filter(mode != "fp32")
    for nq in (1, 4, 64, 1024):
        q = qall[:nq].contiguous()
        reps = 10 if nq <= 64 else 3
        for rank in (10, 100, 1000, 10000, 100000):
            t = thr[rank][:nq].contiguous()
            k = min(rank, 512)
            base_ms = timed(lambda: idx.search_flat(q, k, stream=st), reps)
            for mr in (100, 16384):
                for name in ("flat_thr_scan", "flat_thr_select", "flat_thr_gemm", "flat_thr_rescore"):
                    ctx.profile_read(name)
                ms = timed(lambda: idx.search_flat_threshold(q, t, mr, stream=st), reps)
                f0 = idx.flat_stats()
                ctx.profile_enable(True)
                _, _, cnt = idx.search_flat_threshold(q, t, mr, stream=st)
                torch.cuda.synchronize()
                ctx.profile_enable(False)
                ls, scan_ms = ctx.profile_read("flat_thr_scan")
                lsel, sel_ms = ctx.profile_read("flat_thr_select")
                _, gemm_ms = ctx.profile_read("flat_thr_gemm")
                _, rs_ms = ctx.profile_read("flat_thr_rescore")
                f1 = idx.flat_stats()
                print(f"{mode:11s} nq={nq:5d} rank={rank:6d} max_results={mr:6d}: {ms:8.3f} ms  (scan {scan_ms:7.3f} ms in {ls} passes, "
                      f"gemm {gemm_ms:7.3f} ms, rescore {rs_ms:7.3f} ms, select {sel_ms:7.3f} ms; fall-backs {f1[1] - f0[1]}; mean count {cnt.float().mean().item():8.1f})  vg_search_flat k={k}: {base_ms:7.3f} ms  "
                      f"ratio {ms / base_ms:5.2f}", flush=True)
idx.enable_bf16_filter(False)
