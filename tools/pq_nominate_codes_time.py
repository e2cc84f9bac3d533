"""vg_search_pq_adc, nq queries x rows x 768 (m = 96, K = 256): the table scan, the nomination on the image of the decoded rows
(vg_index_enable_pq_nomination, mode 1) and the nomination from the codes (vg_index_enable_pq_nomination_from_codes, mode 2) —
ms per call, the GEMM's share from the profile scopes, what each mode keeps resident, and equality of the results.
    python tools/pq_nominate_codes_time.py [rows] [small | filtered]
filtered: search_flat_filtered (scan = PQ) batches under a row filter — one for the batch keeping 100 %, 10 % or 1 % of the rows, or one
per query keeping 10 % — over 100k and 1M rows: the filtered scan (mode 3 without on & 4) against the filtered nomination (mode 7).
Above 2M rows: one pass, 1024 queries, k = 10, the scan against mode 2 (the image would be 16x the codes).
small: the batches of 8 .. 128 queries that mode 2 takes when enabled with small_batches (info mode 3, flat_gemm_pq_small_kernel)
instead — segments of 100k, 1M and (rows >= 10000000) 10M rows, k = 10 (128 x 1M: k = 100 too), the scan against mode 3 and the
image mode, the three legs alternating on one index in windows of ~300 ms, every shape warmed, the median of 5 windows with their
min and max: where kPqNomCodesSmallMinPairs comes from."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench
ctx = vg.Context(0); dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
SMALL = "small" in sys.argv[2:]
big = n > 2_000_000 and not SMALL
rows = bench.gen_rows(0, n, dev)
q = bench.gen_queries(2, dev)[0]
st = torch.cuda.current_stream()
pq = vg.ProductQuantizer(ctx, 768, 96, 256)
pq.train(rows[:65536], iters=5)
codes = torch.cat([pq.encode(rows[lo:lo + 1_000_000]) for lo in range(0, n, 1_000_000)]) if SMALL else pq.encode(rows)   # (small: a million at a time)
del rows
from tests import hooks
hooks.set_hook("VG_PQ_NOM_ALWAYS", 1)                  # every batch above 128 queries takes the nomination: where the crossover is
idx = vg.Index(ctx, n, 768)
idx.set_pq_codes(pq, codes)
code_bytes = n * 96
SCOPES = {1: "sq8_nominate_gemm", 2: "pq_codes_gemm"}


def timed(nq, k, reps):
    qs = q[:nq].contiguous()
    for _ in range(2): r = idx.search_pq_adc(qs, k, stream=st)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps): r = idx.search_pq_adc(qs, k, stream=st)
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, r


def mode(md, nq, k, reps):
    """ms per call, ms per GEMM launch, held bytes, results"""
    idx.enable_pq_nomination(False)
    idx.enable_pq_nomination_from_codes(False)
    if md == 0:
        ms, r = timed(nq, k, reps)
        return ms, 0.0, 0, r
    (idx.enable_pq_nomination if md == 1 else idx.enable_pq_nomination_from_codes)(True)
    held = idx.pq_nomination_info()[1]
    ms, r = timed(nq, k, reps)                          # (timed without the profile's events)
    ctx.profile_read(SCOPES[md]); ctx.profile_enable(True)
    idx.search_pq_adc(q[:nq].contiguous(), k, stream=st); torch.cuda.synchronize()
    l, gms = ctx.profile_read(SCOPES[md]); ctx.profile_enable(False)
    return ms, gms / max(l, 1), held, r


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def small_shape(ix, rows_n, nq, k, windows=5):
    """one line: the median / min / max ms per call of each leg, the GEMM's own ms per call, equality with the scan"""
    qs = q[:nq].contiguous()
    legs = {0: "scan", 3: "mode 3", 1: "image"}
    scope = {3: "pq_codes_gemm_small", 1: "sq8_nominate_gemm"}

    def switch(md):
        ix.enable_pq_nomination(False)
        ix.enable_pq_nomination_from_codes(False)
        if md:
            ix.enable_pq_nomination(True) if md == 1 else ix.enable_pq_nomination_from_codes(True, small_batches=True)

    ms, res, gemm = {md: [] for md in legs}, {}, {}
    for w in range(windows + 1):                        # the legs alternate; the first round warms up
        for md in legs:
            switch(md)
            est = 0.012 * nq * rows_n / 1e6 + 0.1 if md == 0 else 0.3 + 0.3 * rows_n / 1e6   # ms a call, roughly
            reps = max(3, int(300 / est))                  # ~300 ms a window
            r = ix.search_pq_adc(qs, k, stream=st)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps): r = ix.search_pq_adc(qs, k, stream=st)
            e1.record(st); torch.cuda.synchronize()
            if w:
                ms[md].append(e0.elapsed_time(e1) / reps)
            res[md] = r
            if md and w == windows:                     # the GEMM's own time: ten calls under the profile's events
                ctx.profile_read(scope[md]); ctx.profile_enable(True)
                for _ in range(10): ix.search_pq_adc(qs, k, stream=st)
                torch.cuda.synchronize()
                gemm[md] = ctx.profile_read(scope[md])[1] / 10; ctx.profile_enable(False)
    txt = "  ".join(f"{legs[md]} {statistics.median(ms[md]):8.3f} [{min(ms[md]):.3f} {max(ms[md]):.3f}]" for md in legs)
    print(f"{rows_n:9d} rows k {k:3d} {nq:4d} queries: {txt}  GEMM mode 3 {gemm[3]:6.3f} image {gemm[1]:6.3f} ms/call  "
          f"scan / mode 3 {statistics.median(ms[0]) / statistics.median(ms[3]):5.2f}  bits equal: {same(res[0], res[3])} {same(res[0], res[1])}", flush=True)


def packed_masks(count, rows_n, keep):
    """count filters of rows_n rows (rows_n % 8 == 0) keeping a share `keep` of them, as packed bits on the device"""
    w = (1 << torch.arange(8, device=dev)).to(torch.int32)
    out = torch.empty((count, rows_n // 8), dtype=torch.uint8, device=dev)
    for lo in range(0, count, 64):
        b = (torch.rand((min(64, count - lo), rows_n // 8, 8), device=dev) < keep).to(torch.int32)
        out[lo:lo + 64] = (b * w).sum(-1).to(torch.uint8)
    return out


def filtered_shape(ix, rows_n, nq, k, mask, what, windows=5):
    """one line: search_flat_filtered (scan = PQ) under mode 3 without the flag (the filtered scan) and with it (mode 7), alternating
    windows of ~100 ms; the GEMM's own ms per call from its scope, whether a scan kernel ran beside it (queries rescanned), equality"""
    qs = q[:nq].contiguous()
    scope = "pq_codes_gemm_small" if nq <= 128 else "pq_codes_gemm"
    search = lambda: ix.search_flat_filtered(qs, k, mask, scan=1, stream=st)
    ms, res = {0: [], 1: []}, {}
    for w in range(windows + 1):                        # the legs alternate; the first round warms up
        for md in (0, 1):
            ix.enable_pq_nomination_from_codes(True, small_batches=True, filtered=bool(md))
            reps = max(1, int(100 / (25e-9 * nq * rows_n + 0.05 if md == 0 else 0.3 + 1.5e-9 * nq * rows_n)))
            res[md] = search()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps): res[md] = search()
            e1.record(st); torch.cuda.synchronize()
            if w:
                ms[md].append(e0.elapsed_time(e1) / reps)
    for s in (scope, "pq_adc_scan", "pq_adc_probe"): ctx.profile_read(s)
    ctx.profile_enable(True)
    for _ in range(10): search()
    torch.cuda.synchronize()
    gemm = ctx.profile_read(scope)[1] / 10
    rescans = ctx.profile_read("pq_adc_scan")[0] + ctx.profile_read("pq_adc_probe")[0]
    ctx.profile_enable(False)
    line = f"{rows_n:8d} rows  k {k:3d}  {nq:5d} queries  {what}:"
    for md, name in ((0, "scan"), (1, "nominated")):
        line += f"  {name} {statistics.median(ms[md]):8.3f} ms [{min(ms[md]):.3f} .. {max(ms[md]):.3f}]"
    print(line + f"  (GEMM {gemm:6.3f} ms, scan launches in 10 nominated calls {rescans}, bits equal: {same(res[0], res[1])})"
          f"  scan / nominated {statistics.median(ms[0]) / statistics.median(ms[1]):5.2f}", flush=True)


if "filtered" in sys.argv[2:]:
    # filtered: where kPqNomCodesMaskedMinPairs and kPqNomCodesMaskedSmall* come from (profiles/pq_nominate_codes_time_filtered.txt)
    del idx
    for rows_n in (100_000, 1_000_000):
        ix = vg.Index(ctx, rows_n, 768)
        ix.set_pq_codes(pq, codes[:rows_n].contiguous())
        batch = {keep: packed_masks(1, rows_n, keep)[0] for keep in (0.1, 0.01)}
        batch[1.0] = torch.full((rows_n // 8,), 255, dtype=torch.uint8, device=dev)
        per_query = packed_masks(1024 if rows_n == 1_000_000 else 129, rows_n, 0.1)
        kinds = (1.0, 0.1, 0.01, "q")
        if rows_n == 100_000:
            plan = [(nq, 10, kind) for nq in (32, 128) for kind in kinds] + [(129, 10, 0.1)]
        else:
            plan = [(nq, 10, kind) for nq in (8, 32, 128) for kind in kinds] + [(129, 10, 0.1), (129, 10, 0.01), (256, 10, 0.01)]
            plan += [(1024, 10, kind) for kind in kinds] + [(1024, 100, 0.1)]
        print(f"{rows_n} rows x 768, m 96: codes {rows_n * 96 / 1e6:.1f} MB, filtered", flush=True)
        for nq, k, kind in plan:
            mask, what = (per_query[:nq], "per query 10 %") if kind == "q" else (batch[kind], f"batch {100 * kind:5.1f} %")
            filtered_shape(ix, rows_n, nq, k, mask, what)
        del ix
    sys.exit(0)
if SMALL:
    del idx
    for rows_n in (100_000, 1_000_000, 10_000_000):
        if rows_n > n:
            continue
        ix = vg.Index(ctx, rows_n, 768)
        ix.set_pq_codes(pq, codes[:rows_n].contiguous())
        for nq, k in [(nq, 10) for nq in (8, 32, 64, 96, 128)] + ([(128, 100)] if rows_n == 1_000_000 else []):
            small_shape(ix, rows_n, nq, k)
        del ix
    sys.exit(0)
print(f"{n} rows x 768, m 96: codes {code_bytes / 1e6:.1f} MB", flush=True)
for k in ((10,) if big else (10, 100)):
    for nq in ((1024,) if big else (129, 256, 512, 1024)):
        ms0, _, _, r0 = mode(0, nq, k, 2 if big else 3)
        ms2, g2, held2, r2 = mode(2, nq, k, 3 if big else 5)
        line = (f"k {k:3d}  {nq:5d} queries: scan {ms0:8.3f} ms, from codes {ms2:8.3f} ms (GEMM {g2:6.3f} ms, held {held2 / 1e6:8.2f} MB = "
                f"{held2 / code_bytes:5.3f}x codes), bits equal: {same(r0, r2)}")
        if not big:
            ms1, g1, held1, r1 = mode(1, nq, k, 5)
            line += (f"; image {ms1:8.3f} ms (GEMM {g1:6.3f} ms, held {held1 / 1e6:8.2f} MB = {held1 / code_bytes:5.2f}x codes), bits equal: "
                     f"{same(r0, r1)}; from codes / image {ms2 / ms1:5.2f}")
        print(line, flush=True)
