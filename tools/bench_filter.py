"""vg_filter_evaluate at the size the filtered searches run at: ROWS rows (default 1M), 1024 queries, each with two range
clauses on two f64 fields at about 10 % selectivity each (~1 % together).  Three figures from one run:
  evaluate_ms   vg_filter_evaluate with every buffer (clauses, offsets, masks, counts) on the device: device events around
                each call, median of REPS calls after WARMUP
  h2d_ms        the host-to-device copy of the same nq x ceil(rows / 8) bytes of masks from pinned host memory (device events,
                median): the part of a host-evaluated filter's path that no host speed-up removes
  numpy_ms      numpy evaluating the same filters on the usable cores (a thread pool of min(16, the CPUs this process may run
                on); numpy's compares and packbits release the interpreter lock), wall time of the whole batch, once
and the same evaluate call at nq = 1 and nq = 32 (where a single query's filter may be better served by the reference's
sorted-column binary search, numeric_index.go:501-532, than by a column scan).  floor_ms is the bytes the kernel must move
(the two columns once, the masks once) over the measured streaming rate of the chip (STREAM_TBS); floor_fraction =
floor_ms / evaluate_ms.  The device masks are compared with numpy's, bit for bit, before anything is reported.
One JSON line.  A run without a GPU fails.
Usage: python tools/bench_filter.py [rows] [nq]"""
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STREAM_TBS = 6.29   # float4 copy on an MI355X: the rate a streaming kernel can reach
WARMUP, REPS = 3, 20


def main():
    import torch

    import vecgo_amd as vg
    from vecgo_amd._lib import check
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter: no GPU")
    rng = np.random.default_rng(1)
    v0, v1 = rng.random(rows), rng.random(rows)
    lo = 0.08 + 0.04 * rng.random(nq)            # field 0 <  lo: 8 .. 12 % of the rows
    hi = 0.92 - 0.04 * rng.random(nq)            # field 1 >= hi: 8 .. 12 %
    fsets = [[(0, "lt", float(lo[q])), (1, "gte", float(hi[q]))] for q in range(nq)]
    ctx = vg.Context(0)
    cols = vg.Columns(ctx, rows)
    cols.set_f64(0, v0)
    cols.set_f64(1, v1)
    nbytes = (rows + 7) // 8
    stride = (nbytes + 7) // 8 * 8
    clauses, off, _ = vg.pack_filter_sets(fsets)
    d_cl = torch.from_numpy(clauses.view(np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off).cuda()
    mask = torch.zeros((nq, stride), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(nq, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream if stream.cuda_stream else 1)

    def evaluate(n):
        check(cols._lib.vg_filter_evaluate(cols._h, C.c_void_p(d_cl.data_ptr()), C.c_void_p(d_off.data_ptr()), C.c_int64(n), None,
                                              C.c_int64(0), None, C.c_void_p(mask.data_ptr()), C.c_int64(stride),
                                              C.c_void_p(counts.data_ptr()), sp))

    def timed(fn, reps):
        ms = []
        for i in range(WARMUP + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    ev = {n: timed(lambda n=n: evaluate(n), REPS) for n in (1, 32, nq)}
    evaluate(nq)
    torch.cuda.synchronize()
    got = mask.cpu().numpy()[:, :nbytes]
    got_counts = counts.cpu().numpy()

    # the same filters in numpy on the usable cores
    workers = min(16, len(os.sched_getaffinity(0)))
    want = np.empty((nq, nbytes), np.uint8)

    def host_eval(q):
        want[q] = np.packbits((v0 < lo[q]) & (v1 >= hi[q]), bitorder="little")
    t0 = time.perf_counter()
    with ThreadPoolExecutor(workers) as pool:
        list(pool.map(host_eval, range(nq)))
    numpy_ms = (time.perf_counter() - t0) * 1e3
    if not np.array_equal(got, want):
        raise SystemExit("bench_filter: the device masks differ from numpy's")
    if not np.array_equal(got_counts, np.unpackbits(want, axis=1).sum(axis=1)):
        raise SystemExit("bench_filter: the device counts differ from numpy's")

    pinned = torch.from_numpy(want).pin_memory()
    dst = torch.empty((nq, nbytes), dtype=torch.uint8, device="cuda")
    h2d = timed(lambda: dst.copy_(pinned, non_blocking=True), 10)

    moved = 2 * rows * 8 + nq * nbytes
    floor_ms = moved / (STREAM_TBS * 1e12) * 1e3
    print(json.dumps({
        "bench": "filter_evaluate", "rows": rows, "nq": nq, "clauses_per_query": 2, "mean_selectivity": float(got_counts.mean() / rows),
        "evaluate_ms": round(ev[nq][0], 4), "evaluate_ms_min_max": [round(ev[nq][1], 4), round(ev[nq][2], 4)],
        "evaluate_nq1_ms": round(ev[1][0], 4), "evaluate_nq32_ms": round(ev[32][0], 4),
        "h2d_ms": round(h2d[0], 4), "h2d_ms_min_max": [round(h2d[1], 4), round(h2d[2], 4)], "h2d_gbs": round(nq * nbytes / h2d[0] / 1e6, 1),
        "evaluate_over_h2d": round(ev[nq][0] / h2d[0], 4),
        "numpy_ms": round(numpy_ms, 1), "numpy_threads": workers,
        "bytes_moved": moved, "floor_ms": round(floor_ms, 4), "floor_fraction": round(floor_ms / ev[nq][0], 4),
        "device": ctx.device_info()["arch"]}))


if __name__ == "__main__":
    main()
