"""vg_search_rabitq, nq queries x rows x dim: the multi-query scan against the int8 matrix-core nomination
(vg_index_enable_rabitq_nomination) — ms per call (the median of several timed windows, with their min and max: the run's spread),
the nomination's stage split from the profile scopes (threshold sample, GEMM, verify; the rescans' scan), the queries the scan had
to answer again, and equality of the results.
    python tools/rabitq_nominate_time.py [max_rows]
dim 768: 129, 256 and 1024 queries x 100k, 1M (and with max_rows >= 10000000: 10M) rows at k = 10 and 100; dim 128 and 1536 at
1024 x 1M.  The two legs of a shape alternate inside one run.  The scan is the library's own: its 1024 x 10M figure should agree
with the one DESIGN.md section 8 records before the run is trusted."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg
ctx = vg.Context(0); dev = torch.device("cuda", 0)
max_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
st = torch.cuda.current_stream()
from tests import hooks
hooks.set_hook("VG_RABITQ_NOM_ALWAYS", 1)               # every batch above 128 queries takes the mode: where the crossover is
STAGES = ("rabitq_nom_sample", "rabitq_nom_gemm", "rabitq_nom_verify", "rabitq_scan_mq")


def encoded(n, dim, seed):
    """RaBitQ codes of n i.i.d. normal rows, encoded block by block (the rows are never resident together)"""
    rq = vg.RaBitQuantizer(ctx, dim)
    out = torch.empty((n, rq.bytes_total()), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev); g.manual_seed(seed)
    for s in range(0, n, 262144):
        e = min(n, s + 262144)
        rq.encode(torch.randn((e - s, dim), generator=g, device=dev, dtype=torch.float32), out=out[s:e])
    return out


def window(idx, qs, k, reps):
    r = idx.search_rabitq(qs, k, stream=st)              # (the first call after a mode switch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps): r = idx.search_rabitq(qs, k, stream=st)
    e1.record(st); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, r


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def shape(idx, n, dim, qs, k, windows=5):
    nq = qs.shape[0]
    ms, res = {0: [], 1: []}, {}
    for w in range(windows + 1):                         # the legs alternate; the first round warms up
        for md in (0, 1):
            idx.enable_rabitq_nomination(bool(md))
            per_call = 2.2e-9 * nq * n * (dim / 768) * ((k + 63) // 64 if md == 0 else 0.3) + 0.2     # ms, roughly
            t, r = window(idx, qs, k, max(1, int(50 / per_call)))
            if w:
                ms[md].append(t)
            res[md] = r
    idx.enable_rabitq_nomination(True)                   # the stages in a call of its own, under the profile's events
    for s in STAGES: ctx.profile_read(s)
    ctx.profile_enable(True)
    idx.search_rabitq(qs, k, stream=st); torch.cuda.synchronize()
    split = {s: ctx.profile_read(s)[1] for s in STAGES}
    ctx.profile_enable(False)
    rescanned = idx.rabitq_nomination_info()[2]
    scan, nom = statistics.median(ms[0]), statistics.median(ms[1])
    print(f"{n:9d} rows dim {dim:4d} k {k:3d} {nq:5d} queries:  scan {scan:8.3f} ms [{min(ms[0]):.3f} .. {max(ms[0]):.3f}]  nomination {nom:8.3f} ms "
          f"[{min(ms[1]):.3f} .. {max(ms[1]):.3f}]  (sample {split[STAGES[0]]:.3f}, GEMM {split[STAGES[1]]:.3f}, verify {split[STAGES[2]]:.3f}, "
          f"rescans' scan {split[STAGES[3]]:.3f} ms; rescanned {rescanned} of {nq}; bits equal: {same(res[0], res[1])})  scan / nomination "
          f"{scan / nom:5.2f}", flush=True)


PLAN = [(768, 100_000, [(129, 10), (256, 10), (1024, 10), (129, 100), (256, 100), (1024, 100)]),
        (768, 1_000_000, [(129, 10), (256, 10), (1024, 10), (129, 100), (256, 100), (1024, 100)]),
        (128, 1_000_000, [(1024, 10)]),
        (1536, 1_000_000, [(1024, 10)]),
        (768, 10_000_000, [(129, 10), (256, 10), (1024, 10), (129, 100), (256, 100), (1024, 100)])]
codes = {}
for dim, n, shapes in PLAN:
    if n > max_rows:
        continue
    if dim not in codes or codes[dim].shape[0] < n:
        codes[dim] = encoded(max(n, max_rows if dim == 768 else n), dim, 7 + dim)
    g = torch.Generator(device=dev); g.manual_seed(99 + dim)
    q = torch.randn((1024, dim), generator=g, device=dev, dtype=torch.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_rabitq_codes(codes[dim][:n].contiguous())
    print(f"{n} rows x {dim}: codes {codes[dim][:n].numel() / 1e6:.1f} MB", flush=True)
    for nq, k in shapes:
        shape(idx, n, dim, q[:nq].contiguous(), k)
    idx.close()
