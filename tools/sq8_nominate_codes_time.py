"""vg_search_sq8, nq queries x rows x 768: the multi-query scan, the nomination on the image of the dequantised rows
(vg_index_enable_sq8_nomination, mode 1) and the nomination from the codes (vg_index_enable_sq8_nomination_from_codes, mode 2) —
ms per call (the median of several timed windows, with their min and max: the run's spread), the GEMM's share from the profile
scopes, what each mode keeps resident, the queries the scan had to answer again, and equality of the results.
    python tools/sq8_nominate_codes_time.py [max_rows]
Segments of 100k, 300k and 1M rows, and of 4M with max_rows >= 4000000; the legs of a shape alternate inside one run."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench
ctx = vg.Context(0); dev = torch.device("cuda", 0)
max_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rows = bench.gen_rows(0, max(max_rows, 1_000_000), dev)
q = bench.gen_queries(2, dev)[0]
st = torch.cuda.current_stream()
sq = vg.ScalarQuantizer(ctx, 768)
sq.train(rows[:65536])
codes = sq.encode(rows)
del rows
from tests import hooks
hooks.set_hook("VG_SQ8_NOM_CODES_ALWAYS", 1)           # every batch above 128 queries takes mode 2: where the crossover is
SCOPES = {1: "sq8_nominate_gemm", 2: "sq8_codes_gemm"}
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
        (idx.enable_sq8_nomination if md == 1 else idx.enable_sq8_nomination_from_codes)(True)


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def shape(idx, n, nq, k, legs, windows=5):
    qs = q[:nq].contiguous()
    ms, res, held, gemm, rescanned = {m: [] for m in legs}, {}, {}, {}, {}
    for w in range(windows + 1):                        # the legs alternate; the first round warms up
        for md in legs:
            switch(idx, md)
            reps = max(1, int(20 / (45e-9 * nq * n * (1 if md == 0 else 0.05) + 0.2)))   # ~20 ms a window, at least one call
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


PLAN = [(100_000, [(129, 10), (257, 10), (1024, 10)]),
        (300_000, [(129, 10), (257, 10)]),
        (1_000_000, [(129, 10), (257, 10), (1024, 10), (1024, 100)]),
        (4_000_000, [(1024, 10)])]
for n, shapes in PLAN:
    if n > codes.shape[0]:
        continue
    idx = vg.Index(ctx, n, 768)
    idx.set_sq8_codes(sq, codes[:n].contiguous())
    print(f"{n} rows x 768: codes {n * 768 / 1e6:.1f} MB", flush=True)
    for nq, k in shapes:
        shape(idx, n, nq, k, (0, 1, 2))
    idx.close()
