"""vg_search_int4, nq queries x rows x 768: the multi-query scan against the nomination from the nibble codes
(vg_index_enable_int4_nomination) in the same run on the same index — ms per call (the median of several timed windows, with their
min and max: the run's spread), the GEMM's share from the profile scope, what the mode keeps resident, the queries the scan had to
answer again, and equality of the results.  Last, the SQ8 nomination from the codes at 1024 x 1M, k = 10, for the comparison the
two tiles invite (the same tile, half the fill bytes).
    python tools/int4_nominate_time.py [max_rows] [small | filtered]
Segments of 100k and 1M rows, and of 10M with max_rows >= 10000000 (the rows are encoded a million at a time).
small: the batches of 8 .. 128 queries that the mode takes when enabled with small_batches (flat_gemm_int4_small_kernel) instead —
windows of ~300 ms, the GEMM's share from its own profile scope, no SQ8 comparison: where kInt4NomSmallMinPairs comes from.
filtered: batches under a row filter (on | 4) — one for the batch keeping 100 %, 10 % or 1 % of the rows, or one per query keeping
10 % — the filtered scan against the filtered nomination, windows of ~100 ms; batches up to 128 queries with small_batches.  After
the keep-all lines the unfiltered nominated call of the same shape, and the ratio: where kInt4NomMaskedMinPairs and
kInt4NomMaskedSmallMinPairs come from (profiles/int4_nominate_time_filtered.txt)."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench
ctx = vg.Context(0); dev = torch.device("cuda", 0)
max_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
SMALL = "small" in sys.argv[2:]
FILTERED = "filtered" in sys.argv[2:]
WINDOW_MS = 300 if SMALL else 100 if FILTERED else 20
q = bench.gen_queries(2, dev)[0]
st = torch.cuda.current_stream()
iq = vg.Int4Quantizer(ctx, 768)
iq.train(bench.gen_rows(0, 65536, dev))
codes = torch.empty((max(max_rows, 1_000_000), 384), dtype=torch.uint8, device=dev)
for lo in range(0, codes.shape[0], 1_000_000):
    iq.encode(bench.gen_rows(lo, min(lo + 1_000_000, codes.shape[0]), dev), out=codes[lo:lo + 1_000_000])
from tests import hooks
hooks.set_hook("VG_INT4_NOM_ALWAYS", 1)                  # every batch above 128 queries takes the mode: where the crossover is
hooks.set_hook("VG_SQ8_NOM_CODES_ALWAYS", 1)
SCOPE = "int4_codes_gemm_small" if SMALL else "int4_codes_gemm"


def packed_masks(count, n, keep):
    """count filters of n rows (n % 8 == 0) keeping a share `keep` of them, as packed bits on the device"""
    w = (1 << torch.arange(8, device=dev)).to(torch.int32)
    out = torch.empty((count, n // 8), dtype=torch.uint8, device=dev)
    for lo in range(0, count, 64):
        bits = (torch.rand((min(64, count - lo), n // 8, 8), device=dev) < keep).to(torch.int32)
        out[lo:lo + 64] = (bits * w).sum(-1).to(torch.uint8)
    return out


def window(search, qs, k, reps):
    r = search(qs, k, stream=st)                         # (the first call after a mode switch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps): r = search(qs, k, stream=st)
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, r


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def shape(idx, n, nq, k, windows=5, mask=None, what=""):
    qs = q[:nq].contiguous()
    small, scope = (nq <= 128, "int4_codes_gemm_small" if nq <= 128 else "int4_codes_gemm") if FILTERED else (SMALL, SCOPE)
    search = (lambda a, b, stream: idx.search_int4(a, b, mask=mask, stream=stream)) if mask is not None else idx.search_int4
    ms, res = {0: [], 1: []}, {}
    for w in range(windows + 1):                         # the legs alternate; the first round warms up
        for md in (0, 1):
            idx.enable_int4_nomination(bool(md), small_batches=small, filtered=FILTERED)
            reps = max(1, int(WINDOW_MS / (55e-9 * nq * n * (1 if md == 0 else 0.05) + 0.2)))   # ~WINDOW_MS a window, at least one call
            t, res[md] = window(search, qs, k, reps)
            if w:
                ms[md].append(t)
    held = idx.int4_nomination_info()[1]
    ctx.profile_read(scope); ctx.profile_enable(True)    # the GEMM's time in a run of its own, under the profile's events
    search(qs, k, stream=st); torch.cuda.synchronize()
    l, gms = ctx.profile_read(scope); ctx.profile_enable(False)
    rescanned = idx.int4_nomination_info()[2]            # (of the calls since the mode was last enabled; the queries of one call fail alike)
    calls = max(1, int(WINDOW_MS / (55e-9 * nq * n * 0.05 + 0.2))) + 2
    line = f"{n:8d} rows  k {k:3d}  {nq:5d} queries{what}:"
    for md, name in ((0, "scan"), (1, "nominated")):
        line += f"  {name} {statistics.median(ms[md]):8.3f} ms [{min(ms[md]):.3f} .. {max(ms[md]):.3f}]"
    line += f" (GEMM {gms / max(l, 1):6.3f} ms, held {held / 1e6:7.2f} MB, rescanned {rescanned // calls} of {nq}, bits equal: {same(res[0], res[1])})"
    print(line + f"  scan / nominated {statistics.median(ms[0]) / statistics.median(ms[1]):5.2f}", flush=True)
    return statistics.median(ms[1])


def filtered_leg():
    """the shapes of the filtered leg on one index per segment size, every filter kind its own line"""
    for n in (100_000, 1_000_000):
        idx = vg.Index(ctx, n, 768)
        idx.set_int4_codes(iq, codes[:n])
        batch = {keep: packed_masks(1, n, keep)[0] for keep in (0.1, 0.01)}
        batch[1.0] = torch.full((n // 8,), 255, dtype=torch.uint8, device=dev)
        per_query = packed_masks(1024 if n == 1_000_000 else 129, n, 0.1)
        plan = [(nq, 10, kind) for nq in (8, 32, 128) for kind in (1.0, 0.1, 0.01, "q")]
        plan += [(129, 10, 0.1)] if n == 100_000 else [(1024, 10, kind) for kind in (1.0, 0.1, 0.01, "q")] + [(1024, 100, 0.1)]
        print(f"{n} rows x 768: codes {n * 384 / 1e6:.1f} MB, filtered", flush=True)
        for nq, k, kind in plan:
            mask, what = (per_query[:nq], "  per query 10 %") if kind == "q" else (batch[kind], f"  batch {100 * kind:5.1f} %")
            t = shape(idx, n, nq, k, mask=mask, what=what)
            if kind == 1.0:                              # the same shape without a filter, nominated: what the filter's bits cost
                idx.enable_int4_nomination(True, small_batches=nq <= 128, filtered=True)
                reps = max(1, int(WINDOW_MS / (55e-9 * nq * n * 0.05 + 0.2)))
                u = statistics.median([window(idx.search_int4, q[:nq].contiguous(), k, reps)[0] for _ in range(6)][1:])
                print(f"{n:8d} rows  k {k:3d}  {nq:5d} queries  no filter:  nominated {u:8.3f} ms  keep-all / no filter {t / u:5.2f}", flush=True)
        idx.close()


if FILTERED:
    filtered_leg()
    sys.exit(0)


PLAN = [(100_000, [(129, 10), (1024, 10)]), (1_000_000, [(1024, 10), (1024, 100)]), (10_000_000, [(1024, 10)])]
if SMALL:
    PLAN = [(n, [(nq, 10) for nq in (8, 32, 64, 96, 128)] + ([(128, 100)] if n == 1_000_000 else [])) for n in (100_000, 1_000_000, 10_000_000)]
int4_ms = None
for n, shapes in PLAN:
    if n > codes.shape[0]:
        continue
    idx = vg.Index(ctx, n, 768)
    idx.set_int4_codes(iq, codes[:n])
    print(f"{n} rows x 768: codes {n * 384 / 1e6:.1f} MB", flush=True)
    for nq, k in shapes:
        t = shape(idx, n, nq, k)
        if (n, nq, k) == (1_000_000, 1024, 10):
            int4_ms = t
    idx.close()
del codes
if SMALL:
    sys.exit(0)
rows = bench.gen_rows(0, 1_000_000, dev)
sq = vg.ScalarQuantizer(ctx, 768)
sq.train(rows[:65536])
idx = vg.Index(ctx, 1_000_000, 768)
idx.set_sq8_codes(sq, sq.encode(rows))
del rows
idx.enable_sq8_nomination_from_codes(True)
sq8 = [window(idx.search_sq8, q[:1024].contiguous(), 10, 10)[0] for _ in range(6)][1:]
print(f" 1000000 rows  k  10   1024 queries:  SQ8 from the codes {statistics.median(sq8):8.3f} ms [{min(sq8):.3f} .. {max(sq8):.3f}]"
      f"  INT4 / SQ8 {int4_ms / statistics.median(sq8):5.2f}", flush=True)
