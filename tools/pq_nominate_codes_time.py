"""vg_search_pq_adc, nq queries x rows x 768 (m = 96, K = 256): the table scan, the nomination on the image of the decoded rows
(vg_index_enable_pq_nomination, mode 1) and the nomination from the codes (vg_index_enable_pq_nomination_from_codes, mode 2) —
ms per call, the GEMM's share from the profile scopes, what each mode keeps resident, and equality of the results.
    python tools/pq_nominate_codes_time.py [rows]
Above 2M rows: one pass, 1024 queries, k = 10, the scan against mode 2 (the image would be 16x the codes)."""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg, bench
ctx = vg.Context(0); dev = torch.device("cuda", 0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
big = n > 2_000_000
rows = bench.gen_rows(0, n, dev)
q = bench.gen_queries(2, dev)[0]
st = torch.cuda.current_stream()
pq = vg.ProductQuantizer(ctx, 768, 96, 256)
pq.train(rows[:65536], iters=5)
codes = pq.encode(rows)
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
