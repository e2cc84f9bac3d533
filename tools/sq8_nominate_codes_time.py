"""vg_search_sq8, nq queries x rows x 768: the multi-query scan, the nomination on the image of the dequantised rows
(vg_index_enable_sq8_nomination, mode 1) and the nomination from the codes (vg_index_enable_sq8_nomination_from_codes, mode 2) —
ms per call (the median of several timed windows, with their min and max: the run's spread), the GEMM's share from the profile
scopes, what each mode keeps resident, the queries the scan had to answer again, and equality of the results.
    python tools/sq8_nominate_codes_time.py [max_rows] [small | filtered]
Segments of 100k, 300k and 1M rows, and of 4M with max_rows >= 4000000; the legs of a shape alternate inside one run.
filtered: search_flat_filtered (scan = SQ8) batches under a row filter — one for the batch keeping 100 %, 10 % or 1 % of the rows, or
one per query keeping 10 % — over 100k and 1M rows, L2 (Dot at one shape): the filtered scan (mode 3 without on & 4) against the
filtered nomination (mode 7) in alternating windows of ~200 ms on one index, every shape warmed, the median of 5 windows with their
min and max; then the small tile's GEMM scope at 100 % and 1 % kept — what the skip of emptied code tiles buys: where
kSq8NomCodesMaskedMinPairs and kSq8NomCodesMaskedSmallMinPairs come from.
small: the batches of 8 .. 128 queries that mode 2 takes when enabled with small_batches (info mode 3, flat_gemm_sq8_small_kernel)
instead — segments of 100k, 1M and (max_rows >= 10000000) 10M rows, windows of ~300 ms, the scan against mode 3 and the image mode:
where kSq8NomCodesSmallMinPairs comes from."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench
ctx = vg.Context(0); dev = torch.device("cuda", 0)
max_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
SMALL = "small" in sys.argv[2:]
WINDOW_MS = 300 if SMALL else 20
rows = bench.gen_rows(0, max(max_rows, 1_000_000), dev)
q = bench.gen_queries(2, dev)[0]
st = torch.cuda.current_stream()
sq = vg.ScalarQuantizer(ctx, 768)
sq.train(rows[:65536])
codes = torch.cat([sq.encode(rows[lo:lo + 1_000_000]) for lo in range(0, rows.shape[0], 1_000_000)])   # (a million at a time)
del rows
from tests import hooks
hooks.set_hook("VG_SQ8_NOM_CODES_ALWAYS", 1)           # every batch above 128 queries takes mode 2: where the crossover is
SCOPES = {1: "sq8_nominate_gemm", 2: "sq8_codes_gemm_small" if SMALL else "sq8_codes_gemm"}
NAMES = {0: "scan", 1: "image", 2: "from codes"}


def window(idx, qs, k, reps):
    r = idx.search_sq8(qs, k, stream=st)                # (the first call after a mode switch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps): r = idx.search_sq8(qs, k, stream=st)
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, r


def switch(idx, md):
    idx.enable_sq8_nomination(False)
    idx.enable_sq8_nomination_from_codes(False)
    if md:
        idx.enable_sq8_nomination(True) if md == 1 else idx.enable_sq8_nomination_from_codes(True, small_batches=SMALL)


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def shape(idx, n, nq, k, legs, windows=5):
    qs = q[:nq].contiguous()
    ms, res, held, gemm, rescanned = {m: [] for m in legs}, {}, {}, {}, {}
    for w in range(windows + 1):                        # the legs alternate; the first round warms up
        for md in legs:
            switch(idx, md)
            reps = max(1, int(WINDOW_MS / (45e-9 * nq * n * (1 if md == 0 else 0.05) + 0.2)))   # ~WINDOW_MS a window, at least one call
            t, r = window(idx, qs, k, reps)
            if w:
                ms[md].append(t)
            res[md] = r
            if md:
                held[md] = idx.sq8_nomination_info()[1]
    for md in legs:                                     # the GEMM's time in a run of its own, under the profile's events
        if md:
            switch(idx, md)
            ctx.profile_read(SCOPES[md]); ctx.profile_enable(True)
            idx.search_sq8(qs, k, stream=st); torch.cuda.synchronize()
            l, gms = ctx.profile_read(SCOPES[md]); ctx.profile_enable(False)
            gemm[md], rescanned[md] = gms / max(l, 1), idx.sq8_nomination_info()[2]
    line = f"{n:8d} rows  k {k:3d}  {nq:5d} queries:"
    for md in legs:
        v = ms[md]
        line += f"  {NAMES[md]} {statistics.median(v):8.3f} ms [{min(v):.3f} .. {max(v):.3f}]"
        if md:
            line += f" (GEMM {gemm[md]:6.3f} ms, held {held[md] / 1e6:9.2f} MB, rescanned {rescanned[md]} of {nq}, bits equal: {same(res[legs[0]], res[md])})"
    if 1 in legs and 2 in legs:
        line += f"  from codes / image {statistics.median(ms[2]) / statistics.median(ms[1]):5.2f}"
    if 0 in legs and 2 in legs:
        line += f"  scan / from codes {statistics.median(ms[0]) / statistics.median(ms[2]):5.2f}"
    print(line, flush=True)


def packed_masks(count, rows_n, keep):
    """count filters of rows_n rows (rows_n % 8 == 0) keeping a share `keep` of them, as packed bits on the device"""
    w = (1 << torch.arange(8, device=dev)).to(torch.int32)
    out = torch.empty((count, rows_n // 8), dtype=torch.uint8, device=dev)
    for lo in range(0, count, 64):
        b = (torch.rand((min(64, count - lo), rows_n // 8, 8), device=dev) < keep).to(torch.int32)
        out[lo:lo + 64] = (b * w).sum(-1).to(torch.uint8)
    return out


def filtered_shape(idx, n, nq, k, mask, what, windows=5, window_ms=200):
    """one line: search_flat_filtered (scan = SQ8) under mode 3 without the flag (the filtered scan) and with it (mode 7), alternating
    windows; the GEMM's own ms per call from its scope, the scan launches beside it (queries rescanned), equality; the GEMM's ms"""
    qs = q[:nq].contiguous()
    scope = "sq8_codes_gemm_small" if nq <= 128 else "sq8_codes_gemm"
    search = lambda: idx.search_flat_filtered(qs, k, mask, scan=idx.SCAN_SQ8, stream=st)
    ms, res = {0: [], 1: []}, {}
    for w in range(windows + 1):                        # the legs alternate; the first round warms up
        for md in (0, 1):
            idx.enable_sq8_nomination_from_codes(True, small_batches=True, filtered=bool(md))
            reps = max(1, int(window_ms / (45e-9 * nq * n + 0.1 if md == 0 else 0.3 + 2e-9 * nq * n)))
            res[md] = search()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps): res[md] = search()
            e1.record(st); torch.cuda.synchronize()
            if w:
                ms[md].append(e0.elapsed_time(e1) / reps)
    for s in (scope, "sq8_scan", "sq8_probe"): ctx.profile_read(s)
    ctx.profile_enable(True)                            # the GEMM's time in a run of its own, under the profile's events
    for _ in range(10): search()
    torch.cuda.synchronize()
    gemm = ctx.profile_read(scope)[1] / 10
    rescans = ctx.profile_read("sq8_scan")[0] + ctx.profile_read("sq8_probe")[0]
    ctx.profile_enable(False)
    line = f"{n:8d} rows  k {k:3d}  {nq:5d} queries  {what}:"
    for md, name in ((0, "scan"), (1, "nominated")):
        line += f"  {name} {statistics.median(ms[md]):8.3f} ms [{min(ms[md]):.3f} .. {max(ms[md]):.3f}]"
    print(line + f"  (GEMM {gemm:6.3f} ms, scan launches in 10 nominated calls {rescans}, bits equal: {same(res[0], res[1])})"
          f"  scan / nominated {statistics.median(ms[0]) / statistics.median(ms[1]):5.2f}", flush=True)
    return gemm


if "filtered" in sys.argv[2:]:
    for metric in (vg.Metric.L2, vg.Metric.DOT):
        for n in (100_000, 1_000_000):
            if metric != vg.Metric.L2 and n != 1_000_000:
                continue
            idx = vg.Index(ctx, n, 768, metric)
            idx.set_sq8_codes(sq, codes[:n].contiguous())
            batch = {keep: packed_masks(1, n, keep)[0] for keep in (0.1, 0.01)}
            batch[1.0] = torch.full((n // 8,), 255, dtype=torch.uint8, device=dev)
            per_query = packed_masks(1024, n, 0.1)
            kinds = (1.0, 0.1, 0.01, "q")
            plan = [(nq, 10, kind) for nq in (1024, 129, 128, 32, 8) for kind in kinds] + ([(1024, 100, 0.1)] if n == 1_000_000 else [])
            if metric != vg.Metric.L2:
                plan = [(nq, 10, kind) for nq in (1024, 32) for kind in (0.1, "q")]
            print(f"{n} rows x 768, {metric.name}: codes {n * 768 / 1e6:.1f} MB, filtered", flush=True)
            gemm = {}
            for nq, k, kind in plan:
                mask, what = (per_query[:nq], "per query 10 %") if kind == "q" else (batch[kind], f"batch {100 * kind:5.1f} %")
                gemm[nq, k, kind] = filtered_shape(idx, n, nq, k, mask, what)
            for nq in (128, 32, 8):                         # what the skip buys: the small tile's GEMM scope, all rows kept against 1 %
                if (nq, 10, 1.0) in gemm:
                    print(f"{n:8d} rows  {nq:5d} queries  sq8_codes_gemm_small: {gemm[nq, 10, 1.0]:6.3f} ms at 100 % kept, "
                          f"{gemm[nq, 10, 0.1]:6.3f} at 10 %, {gemm[nq, 10, 0.01]:6.3f} at 1 %", flush=True)
            idx.close()
    sys.exit(0)
PLAN = [(100_000, [(129, 10), (257, 10), (1024, 10)]),
        (300_000, [(129, 10), (257, 10)]),
        (1_000_000, [(129, 10), (257, 10), (1024, 10), (1024, 100)]),
        (4_000_000, [(1024, 10)])]
if SMALL:
    PLAN = [(n, [(nq, 10) for nq in (8, 32, 64, 96, 128)] + ([(128, 100)] if n == 1_000_000 else [])) for n in (100_000, 1_000_000, 10_000_000)]
for n, shapes in PLAN:
    if n > codes.shape[0]:
        continue
    idx = vg.Index(ctx, n, 768)
    idx.set_sq8_codes(sq, codes[:n].contiguous())
    print(f"{n} rows x 768: codes {n * 768 / 1e6:.1f} MB", flush=True)
    for nq, k in shapes:
        shape(idx, n, nq, k, (0, 1, 2))
    idx.close()
