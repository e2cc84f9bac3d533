"""Building and writing a DiskANN segment at N x 128, r 32, l 64 (default N = 100k), for quantization none / PQ m 16 / RaBitQ /
INT4, in one process:
  stages  the separate calls vg_diskann_build is made of, each timed on the wall: quantize (train + encode + attach), build
          (vg_vamana_build), reorder (vg_vamana_reorder_bfs)
  one     vg_diskann_build as one call on a second index (the same result bit for bit), then vg_segment_write_diskann: write,
          of which crc = the crc32c_device profile scope inside it
The rows start on the GPU.  Prints one JSON line.  Usage: python tools/diskann_build_time.py [rows]"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import vecgo_amd as vg

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
dim, r, l, m, seed = 128, 32, 64, 16, 42
ctx = vg.Context(0)
g = torch.Generator(device="cuda").manual_seed(7)
base = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
base += 2.0 * torch.randn((64, dim), generator=g, device="cuda")[torch.randint(0, 64, (n,), generator=g, device="cuda")]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round((time.perf_counter() - t0) * 1e3, 1)


def quantizer(kind):
    return {"none": None, "pq": vg.ProductQuantizer(ctx, dim, m, 256), "rabitq": vg.RaBitQuantizer(ctx, dim),
            "int4": vg.Int4Quantizer(ctx, dim)}[kind]


def quantize(idx, kind, q):
    if kind == "pq":
        q.train(base, 20, seed)
        idx.set_pq_codes(q, q.encode(base))
    elif kind == "rabitq":
        idx.set_rabitq_codes(q.encode(base))
    elif kind == "int4":
        q.train(base)
        idx.set_int4_codes(q, q.encode(base))


def stages(kind):
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    t = {}
    _, t["quantize_ms"] = wall(lambda: quantize(idx, kind, quantizer(kind)))
    _, t["build_ms"] = wall(lambda: idx.build_vamana(r=r, l=l, alpha=1.2, seed=seed))
    _, t["reorder_ms"] = wall(idx.reorder_vamana_bfs)
    return t, idx


def one_call(kind):
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    _, build_ms = wall(lambda: idx.diskann_build(r, l, 1.2, quantizer(kind), seed=seed))
    ctx.profile_read("crc32c_device")
    ctx.profile_enable(True)
    img, write_ms = wall(lambda: idx.write_diskann_segment(1, l))
    ctx.profile_enable(False)
    return {"diskann_build_ms": build_ms, "write_ms": write_ms, "of_which_crc_ms": round(ctx.profile_read("crc32c_device")[1], 3),
            "image_bytes": len(img)}, img


out = {"rows": n, "dim": dim, "r": r, "l": l}
one_call("none")  # warm-up: code objects, scratch blocks
for kind in ("none", "pq", "rabitq", "int4"):
    t, idx = stages(kind)
    one, img = one_call(kind)
    out[kind] = {**t, **one, "same_image": img == idx.write_diskann_segment(1, l)}
    del img, idx
print(json.dumps(out))
