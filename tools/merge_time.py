"""vg_index_merge at the compaction's size, 1M x 768 fp32 rows, beside a plain device-to-device hipMemcpyAsync of the same
number of live bytes in the same process (the yardstick: a merge reads every live row once and writes it once).  Cases:
  one      one source of 1M rows, nothing deleted (the rows move as they lie)
  eight    8 sources x 125k rows, 10 % of the rows deleted at random
Per case: the wall time of every timed call (bitmaps up, maps down, the row-count read-back and the allocation of the new
rows included: the host's side, and the noisy one), the four kernels by profile scope (merge_count / merge_scan / merge_rank /
merge_gather, device events), the copy's time by device events, and for both the bytes read plus written per second;
kernel and copy figures are medians of seven.  Each case runs in a child process of its own under a time limit; after a
case that fails or runs out of time nothing more is started.  One JSON line per case.
Usage: python tools/merge_time.py [rows]            (python tools/merge_time.py --case NAME [rows] is one child)"""
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CASES = {"one": (1, 0.0), "eight": (8, 0.1)}
KERNELS = ("merge_count", "merge_scan", "merge_rank", "merge_gather")
STEP_SECONDS = 300
DIM = 768


def run_case(name, rows):
    import ctypes as C

    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import vecgo_amd as vg

    n_sources, p = CASES[name]
    ctx = vg.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rng = np.random.default_rng(1)
    per = rows // n_sources
    sources, deleted = [], []
    for _ in range(n_sources):
        x = torch.randn((per, DIM), generator=gen, device="cuda", dtype=torch.float32)
        idx = vg.Index(ctx, per, DIM)
        idx.set_vectors(x)
        sources.append(idx)
        deleted.append(np.packbits(rng.random(per) < p, bitorder="little") if p else None)
        del x
    dead = None if not p else deleted

    def merge():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        merged, old_to_new, _, _ = vg.merge_indexes(ctx, sources, dead)
        ms = (time.perf_counter() - t0) * 1e3
        live = merged.n
        merged.close()
        return ms, live

    merge()                                            # warm-up: scratch blocks, code objects
    wall = [merge() for _ in range(7)]
    live = wall[0][1]
    ctx.profile_enable(True)
    for k in KERNELS:
        ctx.profile_read(k)
    kernel_ms = {k: [] for k in KERNELS}
    launches = {}
    for _ in range(7):
        merge()
        for k in KERNELS:
            count, ms = ctx.profile_read(k)
            launches[k] = count
            kernel_ms[k].append(ms)
    ctx.profile_enable(False)

    # the yardstick: one hipMemcpyAsync, device to device, of the live bytes, timed by events on the same stream
    live_bytes = live * DIM * 4
    src = torch.empty(live_bytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(live_bytes, dtype=torch.uint8, device="cuda")
    with open("/proc/self/maps") as maps:              # the HIP runtime already in the process, not a second one
        runtime = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    assert len(runtime) == 1, runtime
    hip = C.CDLL(runtime[0])
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream()
    copy_ms = []
    for rep in range(8):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        status = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), live_bytes, 3, stream.cuda_stream)   # 3 = hipMemcpyDeviceToDevice
        b.record(stream)
        b.synchronize()
        if status != 0:
            raise RuntimeError(f"hipMemcpyAsync returned {status}")
        if rep:
            copy_ms.append(a.elapsed_time(b))
    assert bool((dst[:: max(1, live_bytes // 1000)] == 1).all())

    def tbps(ms):
        return round(2 * live_bytes / 1e12 / (ms / 1e3), 2)

    def median(v):
        return sorted(v)[len(v) // 2]
    gather = median(kernel_ms["merge_gather"])
    kernels = sum(median(v) for v in kernel_ms.values())
    walls = [round(w[0], 2) for w in wall]
    print(json.dumps({
        "case": name, "sources": n_sources, "rows": per * n_sources, "dim": DIM, "deleted_share": p, "live_rows": live,
        "live_gb": round(live_bytes / 1e9, 3),
        "merge_wall_ms": walls, "merge_wall_median_tbps": tbps(median(walls)),
        "merge_kernels_ms": round(kernels, 3), "merge_kernels_tbps": tbps(kernels),
        "kernel_ms": {k: round(median(v), 3) for k, v in kernel_ms.items()}, "launches": launches,
        "gather_tbps": tbps(gather),
        "memcpy_ms": round(median(copy_ms), 3), "memcpy_tbps": tbps(median(copy_ms)),
        "gather_over_memcpy_rate": round(median(copy_ms) / gather, 2)}))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--case":
        run_case(args[1], int(args[2]) if len(args) > 2 else 1_000_000)
        return 0
    rows = args[:1]
    for name in CASES:
        try:
            done = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--case", name] + rows, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            print(f"merge_time: case {name} ran past {STEP_SECONDS} s; stopping", file=sys.stderr)
            return 124
        if done.returncode != 0:
            print(f"merge_time: case {name} ended with status {done.returncode}; stopping", file=sys.stderr)
            return done.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
