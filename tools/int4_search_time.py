"""vg_search_int4 timed (dim 768): ms per call as the median of at least 20 calls, each between two events on the stream, after one
warm-up call, with the calls' min and max (the run's spread).
    python tools/int4_search_time.py [rows]
  one query, rows x 768, k = 10: the search against vg_int4_l2_distance_batch(precomputed = 1) over the same codes (the same row
    loop with a store in place of the offer), and their ratio; the two scan kernels alone (the profile's events);
  batches, 1024 x rows and 129 x 100k, k = 10 and 100: the call against nq times the one-query search on the same index;
  the crossover: 2 .. 16 queries against nq times the one-query search (where the dispatch switches to the multi-query kernel);
  filtered, 1024 x rows: a batch mask keeping 1 % and one keeping 100 % of the rows against the unfiltered call."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg
ctx = vg.Context(0); dev = torch.device("cuda", 0)
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
DIM = 768
st = torch.cuda.current_stream()


def timed(fn, calls=20):
    fn(); torch.cuda.synchronize()                       # warm-up
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"


def build(n, seed):
    """an index of n i.i.d. normal rows' INT4 codes, trained on the first block, encoded block by block"""
    iq = vg.Int4Quantizer(ctx, DIM)
    g = torch.Generator(device=dev); g.manual_seed(seed)
    codes = torch.empty((n, iq.code_bytes), dtype=torch.uint8, device=dev)
    for s in range(0, n, 262144):
        e = min(n, s + 262144)
        x = torch.randn((e - s, DIM), generator=g, device=dev, dtype=torch.float32)
        if s == 0:
            iq.train(x)
        iq.encode(x, out=codes[s:e])
    idx = vg.Index(ctx, n, DIM)
    idx.set_int4_codes(iq, codes)
    return iq, codes, idx


g = torch.Generator(device=dev); g.manual_seed(5)
q = torch.randn((1024, DIM), generator=g, device=dev, dtype=torch.float32)
for n in (rows, 100_000):
    iq, codes, idx = build(n, 11 + n)
    print(f"{n} rows x {DIM}: codes {codes.numel() / 1e6:.1f} MB", flush=True)
    out1 = (torch.empty((1, 100), dtype=torch.int32, device=dev), torch.empty((1, 100), dtype=torch.float32, device=dev))
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    one = {}
    for k in (10, 100):
        o1 = (out1[0][:, :k].contiguous(), out1[1][:, :k].contiguous())
        one[k] = timed(lambda: idx.search_int4(q[:1], k, out=o1, stream=st))
    base = timed(lambda: iq.l2_distance(q[0], codes, out=dist, stream=st))
    print(f"  one query k 10: search {fmt(one[10])}   distance batch {fmt(base)}   search / batch {one[10][0] / base[0]:.3f}", flush=True)
    print(f"  one query k 100: search {fmt(one[100])}", flush=True)
    for name in ("int4_search_one", "int4_scan"): ctx.profile_read(name)
    ctx.profile_enable(True)                             # the two scan kernels alone, under the profile's events (one call each)
    idx.search_int4(q[:1], 10, stream=st); iq.l2_distance(q[0], codes, out=dist, stream=st); torch.cuda.synchronize()
    ks, kb = ctx.profile_read("int4_search_one")[1], ctx.profile_read("int4_scan")[1]
    ctx.profile_enable(False)
    print(f"  one query k 10, kernels alone: search scan {ks:.3f} ms   distance scan {kb:.3f} ms   ratio {ks / kb:.3f}", flush=True)
    for nq in ((1024, 129) if n == rows else (129,)):
        for k in (10, 100):
            outb = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
            t = timed(lambda: idx.search_int4(q[:nq], k, out=outb, stream=st))
            print(f"  {nq:5d} queries k {k:3d}: batch {fmt(t)}   {nq} x one query {nq * one[k][0]:9.3f} ms   ratio {nq * one[k][0] / t[0]:6.2f}", flush=True)
    for nq in (2, 3, 4, 5, 6, 8, 9, 12, 16):
        outb = (torch.empty((nq, 10), dtype=torch.int32, device=dev), torch.empty((nq, 10), dtype=torch.float32, device=dev))
        t = timed(lambda: idx.search_int4(q[:nq], 10, out=outb, stream=st))
        print(f"  crossover {nq:3d} queries k 10: batch {fmt(t)}   {nq} x one query {nq * one[10][0]:8.3f} ms", flush=True)
    if n == rows:
        nq, k = 1024, 10
        outb = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
        gm = torch.Generator(device=dev); gm.manual_seed(3)
        keep1 = torch.rand(n, generator=gm, device=dev) < 0.01
        for name, keep in (("none", None), ("1 %", keep1), ("100 %", torch.ones(n, dtype=torch.bool, device=dev)), ("none", None)):
            m = None
            if keep is not None:
                pad = (-n) % 8
                bits = torch.cat([keep, torch.zeros(pad, dtype=torch.bool, device=dev)]).view(-1, 8).to(torch.uint8)
                m = (bits << torch.arange(8, device=dev, dtype=torch.uint8)).sum(1).to(torch.uint8).contiguous()
            t = timed(lambda: idx.search_int4(q[:nq], k, mask=m, out=outb, stream=st))
            print(f"  filtered {nq} queries k {k}, batch mask keeps {name:>5}: {fmt(t)}", flush=True)
    idx.close()
