"""vg_search_binary timed (dim 768) against what reads the same bits: ms per call, each call between two events on the stream,
as the median [min .. max] over alternating windows of one run (3 rounds of 7 calls per contender, one warm-up call each), so that
a drift of the machine falls on every contender alike.
    python tools/binary_search_time.py [rows ...]        (default 1000000 10000000 100000)
  one query, k = 10 (the first row count only): the search against vg_binary_hamming_batch over the same codes — the same bytes
    without the selection;
  batches, 1024 queries (129 and 1024 at 100 000 rows), k = 10 and 100: the popcount scan (hook VG_BINARY_NO_NOM) against the
    matrix-core path (VG_BINARY_NOM_ALWAYS) on one index — where the dispatch's crossover comes from —, and against
    vg_search_rabitq on an index of the same rows — the same sign bits plus a float formula — with its nomination off (its
    popcount scan) and on (its int8 tile); `rescanned`: queries of the window the matrix path handed back to the scan."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg
from tests import hooks
ctx = vg.Context(0); dev = torch.device("cuda", 0)
sizes = [int(a) for a in sys.argv[1:]] or [1_000_000, 10_000_000, 100_000]
DIM = 768
st = torch.cuda.current_stream()


def alternate(fns, rounds=3, calls=7, before=None):
    """before[name]: what switches the contender on, run in front of its window (not timed)"""
    ms = {name: [] for name in fns}
    before = before or {}
    for name, fn in fns.items():
        before.get(name, lambda: None)(); fn()               # warm-up
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns.items():
            before.get(name, lambda: None)()
            for _ in range(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st); fn(); e1.record(st); e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def fmt(t):
    return f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"


def build(n, seed):
    """n i.i.d. normal rows as binary codes (threshold 0: the sign bits) and as RaBitQ codes, block by block, an index of each"""
    bq, rq = vg.BinaryQuantizer(ctx, DIM), vg.RaBitQuantizer(ctx, DIM)
    bq.threshold, bq.trained = 0.0, True
    g = torch.Generator(device=dev); g.manual_seed(seed)
    bc = torch.empty((n, bq.words * 8), dtype=torch.uint8, device=dev)
    rc = torch.empty((n, rq.bytes_total()), dtype=torch.uint8, device=dev)
    for s in range(0, n, 262144):
        e = min(n, s + 262144)
        x = torch.randn((e - s, DIM), generator=g, device=dev, dtype=torch.float32)
        bq.encode(x, out=bc[s:e]); rq.encode(x, out=rc[s:e])
    ib, ir = vg.Index(ctx, n, DIM), vg.Index(ctx, n, DIM)
    ib.set_binary_codes(bq, bc); ir.set_rabitq_codes(rc)
    del rc
    return bq, bc, ib, ir


g = torch.Generator(device=dev); g.manual_seed(5)
q = torch.randn((1024, DIM), generator=g, device=dev, dtype=torch.float32)
for i, n in enumerate(sizes):
    bq, bc, ib, ir = build(n, 11 + n)
    print(f"{n} rows x {DIM}: binary codes {bc.numel() / 1e6:.1f} MB", flush=True)
    if i == 0:
        o1 = (torch.empty((1, 10), dtype=torch.int32, device=dev), torch.empty((1, 10), dtype=torch.float32, device=dev))
        dist = torch.empty(n, dtype=torch.int32, device=dev)
        t = alternate({"search": lambda: ib.search_binary(q[:1], 10, out=o1, stream=st),
                       "batch": lambda: bq.compute_hamming_distance(q[0], bc, out=dist, stream=st)})
        print(f"  one query k 10: search {fmt(t['search'])}   hamming batch {fmt(t['batch'])}   search / batch "
              f"{t['search'][0] / t['batch'][0]:.3f}", flush=True)
    for nq, k in [(nq, k) for nq in ((1024,) if n >= 1_000_000 else (129, 1024)) for k in (10, 100)]:
        ob = (torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
        rabitq = lambda: ir.search_rabitq(q[:nq], k, out=ob, stream=st)
        binary = lambda: ib.search_binary(q[:nq], k, out=ob, stream=st)

        def path(name):
            hooks.set_hook("VG_BINARY_NO_NOM", name == "scan"); hooks.set_hook("VG_BINARY_NOM_ALWAYS", name == "matrix")
        r0 = ib.binary_info()[2]
        t = alternate({"binary scan": binary, "binary matrix": binary, "rabitq scan": rabitq, "rabitq nomination": rabitq},
                      before={"binary scan": lambda: path("scan"), "binary matrix": lambda: path("matrix"),
                              "rabitq scan": lambda: ir.enable_rabitq_nomination(False), "rabitq nomination": lambda: ir.enable_rabitq_nomination(True)})
        path("")
        print(f"  {nq:5d} queries k {k:3d}: " + "   ".join(f"{name} {fmt(v)}" for name, v in t.items())
              + f"   rescanned {ib.binary_info()[2] - r0} of {22 * nq}", flush=True)
    ib.close(); ir.close()
    del bc
