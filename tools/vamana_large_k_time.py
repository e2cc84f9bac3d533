"""The Vamana walk at large k: per node scorer (fp32 / PQ / RaBitQ / INT4) and k in {512, 1024, 4096, 16384}, kernel time per
batch of 1 and of 1024 queries, node scores per query and G scores/s, on the layer-0 stand-in graph of tools/vamana_time.py
(vg_hnsw_build over N x 768 i.i.d. normal rows); then the recall@10 the wide walk exists for, over one vg_vamana_build graph
at 200k: top-10 of a walk at k' in {10, 100, 512, 1024, 4096, 16384} against exact vg_search_flat, for fp32 and for a PQ
walk + vg_rerank to 10.  argv: [N [build_n]] (N = 0: the recall curve only)."""
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np, torch
import vecgo_amd as vg, bench

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
BN = int(sys.argv[2]) if len(sys.argv) > 2 else 200_000
D = 768
ctx = vg.Context(0); dev = torch.device("cuda", 0)
st = torch.cuda.current_stream()


def codes_for(idx, rows):
    pq = vg.ProductQuantizer(ctx, D, 96, 256); pq.train(rows[:32768], iters=5, seed=1)
    idx.set_pq_codes(pq, pq.encode(rows))
    rq = vg.RaBitQuantizer(ctx, D); idx.set_rabitq_codes(rq.encode(rows))
    i4 = vg.Int4Quantizer(ctx, D); i4.train(rows[:32768]); idx.set_int4_codes(i4, i4.encode(rows))
    return pq, rq, i4


def timed(fn, reps):
    torch.cuda.synchronize()
    ctx.profile_read("vamana_search"); ctx.profile_enable(True)
    for _ in range(reps): fn()
    torch.cuda.synchronize()
    _, ms = ctx.profile_read("vamana_search"); ctx.profile_enable(False)
    return ms / reps


# ---- 1. time and score rate on the stand-in graph (N = 0: skipped) -------------------------------------------------------
if N > 0:
    rows = bench.gen_rows(0, N, dev)
    idx = vg.Index(ctx, N, D); idx.set_vectors(rows)
    idx.build_hnsw(m=32, ef_construction=300, max_batch=8192, growth_div=32)
    keep = codes_for(idx, rows)
    l0, _, entry = idx.get_hnsw_graph(); idx.set_vamana_graph(l0, entry)
    qall = bench.gen_queries(8, dev).reshape(-1, D)[:1024].contiguous()
    print(f"| kind | k | ms / 1 query | ms / 1024 queries | node scores / query | G scores/s (1024) |")
    print(f"|---|---|---|---|---|---|")
    for kind, name in ((0, "fp32"), (1, "PQ"), (2, "RaBitQ"), (3, "INT4")):
        for k in (512, 1024, 4096, 16384):
            res = {}
            for nq in (1, 1024):
                q = qall[:nq]
                _, _, stats = idx.search_vamana(q, k, kind=kind, stats=True, stream=st)
                reps = 3 if nq == 1024 and k >= 4096 else 5
                ms = timed(lambda: idx.search_vamana(q, k, kind=kind, stream=st), reps)
                res[nq] = (ms, float(stats[:, 1].sum()) / nq)
            ms1, ms1k, dcq = res[1][0], res[1024][0], res[1024][1]
            print(f"| {name} | {k} | {ms1:.2f} | {ms1k:.1f} | {dcq:.0f} | {dcq * 1024 / (ms1k * 1e-3) / 1e9:.2f} |", flush=True)
    del idx, keep, rows, l0
    torch.cuda.empty_cache()

# ---- 2. recall@10 over a vg_vamana_build graph ------------------------------------------------------------------------------
rows = bench.gen_rows(0, BN, dev)
idx = vg.Index(ctx, BN, D); idx.set_vectors(rows)
t0 = time.time(); idx.build_vamana(); torch.cuda.synchronize()
print(f"\nvg_vamana_build over {BN} x {D}: {time.time() - t0:.1f} s")
pq, rq, i4 = codes_for(idx, rows)
q = bench.gen_queries(8, dev).reshape(-1, D)[:256].contiguous()
truth, _ = idx.search_flat(q, 10)
truth = truth.cpu().numpy().astype(np.int64)


def recall(ids):
    ids = ids.cpu().numpy().astype(np.int64)
    return float(np.mean([len(set(ids[i, :10]) & set(truth[i])) / 10 for i in range(truth.shape[0])]))


print("| k' | recall@10 fp32 walk | recall@10 PQ walk + rerank to 10 |")
print("|---|---|---|")
for kk in (10, 100, 512, 1024, 4096, 16384):
    f_ids, _ = idx.search_vamana(q, kk, kind=0, stream=st)
    p_ids, _ = idx.search_vamana(q, kk, kind=1, stream=st)
    r_ids, _ = idx.rerank(q, p_ids, 10, stream=st)      # (VG_INVALID_ID padding is skipped)
    print(f"| {kk} | {recall(f_ids):.3f} | {recall(r_ids):.3f} |", flush=True)
