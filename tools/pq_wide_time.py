"""The PQ flat searches over a table wider than one LDS image: 1M x 1536 at m = 192 (dim / 8, the flat writer's default), random
codes and codebooks, 1024 queries and 1 query, k = 10.  The yardstick is vg_search_pq_adc on the same index (the chunked walk
with no mask); against it: vg_search_flat_filtered under an all-ones, a 10 % and a 1 % mask, vg_search_flat_probed over 122
partitions at nprobes 8, vg_search_flat_probed_threshold at max_results 100 without and with rerank.  Every buffer on the
device, device events around each call: median / min / max of RUNS calls after WARM warm-up calls, and the ratio of the
medians to the yardstick's.  The all-ones filtered ids are compared with the yardstick's first.  One JSON line at the end.
argv: [rows] [queries]"""
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import vecgo_amd as vg

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
NQ = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
DIM, M, K, PARTS, NPROBES, MAX_RESULTS = 1536, 192, 10, 122, 8, 100
WARM, RUNS = 3, 10
dev = torch.device("cuda", 0)
ctx = vg.Context(0)
g = torch.Generator(device=dev).manual_seed(1)
rng = np.random.default_rng(1)

rows = torch.randn((N, DIM), generator=g, device=dev, dtype=torch.float32)
codes = torch.randint(0, 256, (N, M), generator=g, device=dev, dtype=torch.uint8)
pq = vg.ProductQuantizer(ctx, DIM, M, 256)
pq.set_codebooks(rng.integers(-128, 128, M * 256 * (DIM // M)).astype(np.int8), (rng.random(M) * 0.02 + 0.005).astype(np.float32),
                 ((rng.random(M) * 2 - 1) * 0.1).astype(np.float32))
cent = (rng.standard_normal((PARTS, DIM)) * 0.7).astype(np.float32)
cuts = np.sort(rng.choice(np.arange(1, N), PARTS - 1, replace=False))
offsets = np.concatenate([[0], cuts, [N]]).astype(np.uint32)


def make_index(partitioned):
    idx = vg.Index(ctx, N, DIM)
    idx.set_vectors(rows)
    idx.set_pq_codes(pq, codes)
    if partitioned:
        idx.set_partitions(cent, offsets)
    return idx


whole, probed = make_index(False), make_index(True)


def packed(keep):
    bits = torch.rand(N, generator=g, device=dev) < keep if keep < 1.0 else torch.ones(N, dtype=torch.bool, device=dev)
    pad = (-N) % 8
    if pad:
        bits = torch.cat([bits, torch.zeros(pad, dtype=torch.bool, device=dev)])
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
    return (bits.view(-1, 8).to(torch.uint8) * weights).sum(1).to(torch.uint8).contiguous()


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


masks = {"all": packed(1.0), "10%": packed(0.1), "1%": packed(0.01)}
report = {"rows": N, "dim": DIM, "m": M, "k": K, "device": ctx.device_info()}
for nq in sorted({NQ, 1}, reverse=True):
    q = torch.randn((nq, DIM), generator=g, device=dev, dtype=torch.float32)
    yard_ids, _ = whole.search_pq_adc(q, K)
    same = torch.equal(yard_ids, whole.search_flat_filtered(q, K, masks["all"], 0, whole.SCAN_PQ)[0])
    # thresholds at each query's 100th table sum (the paged filtered search gives them): about 100 rows pass without rerank
    thr = whole.search_flat_filtered(q, MAX_RESULTS, masks["all"], 0, whole.SCAN_PQ)[1][:, -1].contiguous()
    inf = torch.full((nq,), float("inf"), device=dev)
    legs = {"pq_adc (yardstick)": lambda: whole.search_pq_adc(q, K)}
    for name, mask in masks.items():
        legs[f"filtered {name}"] = lambda mask=mask: whole.search_flat_filtered(q, K, mask, 0, whole.SCAN_PQ)
    legs[f"probed {NPROBES}/{PARTS}"] = lambda: probed.search_flat_probed(q, K, NPROBES, probed.SCAN_PQ)
    legs["threshold"] = lambda: whole.search_flat_probed_threshold(q, thr, MAX_RESULTS, 0, whole.SCAN_PQ, False)
    legs["threshold rerank"] = lambda: whole.search_flat_probed_threshold(q, inf, MAX_RESULTS, 0, whole.SCAN_PQ, True)
    out = {name: timed(fn) for name, fn in legs.items()}
    base = out["pq_adc (yardstick)"]["median_ms"]
    for name, t in out.items():
        t["ratio"] = t["median_ms"] / base
        print(f"nq={nq:5d}  {name:22s} {t['median_ms']:9.3f} ms  (min {t['min_ms']:.3f}, max {t['max_ms']:.3f})  x{t['ratio']:.2f}", flush=True)
    report[f"nq{nq}"] = {"filtered_all_equals_yardstick": bool(same), **out}
print(json.dumps(report))
