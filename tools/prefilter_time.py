"""vg_search_flat_prefilter next to vg_search_flat_filtered (fp32 scan) on the same resident masks: ROWS x DIM fp32 rows
(default 1M x 768), nq in {1, 16, 256, 1024}, filters keeping 10 %, 1 % and 0.1 % of the rows, as
  shared     one mask for the batch (mask_stride 0): the prefilter stages each listed row in LDS once per query group
  each       one random mask per query
  each_same  the shared mask handed over once per query: the same lists through the per-query kernel, every query gathering
             its rows from the caches on its own — what the shared path would cost without the LDS staging
Device events around each call, median of REPS calls after WARMUP; the prefilter waits for its counts inside the call, so
its figure is the whole call.  floor_ms = the gathered bytes (hits x dim x 4, counted once for a shared mask) over the
chip's streaming rate (STREAM_TBS of tools/bench_filter.py); floor_fraction = floor_ms / prefilter_ms.  The two entries'
ids are compared before a cell is printed.  One JSON line per cell.  A run without a GPU fails.
Usage: python tools/prefilter_time.py [rows] [dim] [k]"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
WARMUP, REPS = 3, 20
BATCHES = (1, 16, 256, 1024)
KEEPS = (0.1, 0.01, 0.001)


def main():
    import torch

    import vecgo_amd as vg
    from bench_filter import STREAM_TBS
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    if not torch.cuda.is_available():
        raise SystemExit("prefilter_time: no GPU")
    torch.manual_seed(1)
    ctx = vg.Context(0)
    x = torch.randn((rows, dim), dtype=torch.float32, device="cuda")
    idx = vg.Index(ctx, rows, dim, vg.Metric.L2)
    idx.set_vectors(x)
    del x
    nq_max = max(BATCHES)
    q = torch.randn((nq_max, dim), dtype=torch.float32, device="cuda")
    nbytes = (rows + 7) // 8
    stride = (nbytes + 7) // 8 * 8
    weights = (2 ** torch.arange(8, device="cuda")).to(torch.uint8)

    def random_masks(n, keep):
        """packed little-endian masks [n, stride] made on the device, 64 at a time"""
        out = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
        for q0 in range(0, n, 64):
            c = min(64, n - q0)
            b = torch.zeros((c, nbytes * 8), dtype=torch.bool, device="cuda")
            b[:, :rows] = torch.rand((c, rows), device="cuda") < keep
            out[q0:q0 + c, :nbytes] = (b.view(c, nbytes, 8).to(torch.uint8) * weights).sum(dim=2, dtype=torch.uint8)
        return out

    def timed(fn):
        ms = []
        for i in range(WARMUP + REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    for keep in KEEPS:
        each = random_masks(nq_max, keep)
        same = each[:1].expand(nq_max, stride).contiguous()
        counts = vg.mask_popcount(ctx, each, rows).cpu().numpy()
        for nq in BATCHES:
            for mode in ("shared", "each", "each_same"):
                if nq == 1 and mode != "each":
                    continue
                masks = each[0] if mode == "shared" else (each[:nq] if mode == "each" else same[:nq])
                qs = q[:nq]
                out_p = (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"))
                out_f = (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"))
                idx.search_flat_prefilter(qs, k, masks, out=out_p)
                idx.search_flat_filtered(qs, k, masks, 0, scan=idx.SCAN_F32, out=out_f)
                torch.cuda.synchronize()
                if not (torch.equal(out_p[0], out_f[0]) and torch.equal(out_p[1], out_f[1])):
                    raise SystemExit(f"prefilter_time: the two entries disagree at keep {keep}, nq {nq}, {mode}")
                pre = timed(lambda: idx.search_flat_prefilter(qs, k, masks, out=out_p))
                flt = timed(lambda: idx.search_flat_filtered(qs, k, masks, 0, scan=idx.SCAN_F32, out=out_f))
                hits = int(counts[0]) if mode != "each" else int(counts[:nq].sum())
                gathered = hits * dim * 4 * (1 if mode == "shared" else (nq if mode == "each_same" else 1))
                floor_ms = gathered / (STREAM_TBS * 1e12) * 1e3
                print(json.dumps({"bench": "prefilter_time", "rows": rows, "dim": dim, "k": k, "keep": keep, "nq": nq, "masks": mode,
                                  "hits_per_query": round(hits / (1 if mode != "each" else nq), 1),
                                  "prefilter_ms": round(pre[0], 4), "prefilter_ms_min_max": [round(pre[1], 4), round(pre[2], 4)],
                                  "filtered_ms": round(flt[0], 4), "filtered_ms_min_max": [round(flt[1], 4), round(flt[2], 4)],
                                  "speedup": round(flt[0] / pre[0], 2), "gathered_bytes": gathered, "floor_ms": round(floor_ms, 5),
                                  "floor_fraction": round(floor_ms / pre[0], 4)}), flush=True)
    print(json.dumps({"bench": "prefilter_time", "done": True, "device": ctx.device_info()["arch"]}))


if __name__ == "__main__":
    main()
