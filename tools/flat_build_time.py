"""Building and writing an IVF flat segment at N x 768, 122 partitions (default N = 1M), the new path against the separate calls
it replaces, in one process, each for quantization none / SQ8 / PQ m 96:
  new   vg_flat_build (stages from its profile scopes: km_assign + km_update = k-means and assignment, flat_build_group,
        flat_build_permute) + vg_segment_write_flat (crc32c_device scope inside it)
  old   vg_kmeans_train + vg_kmeans_assign, torch stable argsort + gather of the rows, vg_index_set_vectors / set_partitions,
        quantizer train + encode + set codes, then a host-side image: rows and codes copied back, sections joined, vg_crc32c
        over the body
and the device CRC against the host CRC over the same row bytes.  The rows start on the GPU in both paths.
Prints one JSON line.  Usage: python tools/flat_build_time.py [rows]"""
import json
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import vecgo_amd as vg
from tests import flat_writer_ref as ref

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
dim, parts, m, seed = 768, 122, 96, 42
ctx = vg.Context(0)
g = torch.Generator(device="cuda").manual_seed(7)
base = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
base += 2.0 * torch.randn((64, dim), generator=g, device="cuda")[torch.randint(0, 64, (n,), generator=g, device="cuda")]
SCOPES = ("km_assign", "km_update", "flat_build_group", "flat_build_permute", "crc32c_device", "pq_kmeanspp", "pq_assign", "pq_update", "pq_encode")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, round((time.perf_counter() - t0) * 1e3, 1)


def quantizer(kind):
    return {"none": None, "sq8": vg.ScalarQuantizer(ctx, dim), "pq": vg.ProductQuantizer(ctx, dim, m, 256)}[kind]


def new_path(kind):
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    for s in SCOPES:
        ctx.profile_read(s)
    ctx.profile_enable(True)
    _, build_ms = wall(lambda: idx.flat_build(parts, quantizer(kind), seed=seed))
    img, write_ms = wall(lambda: idx.write_flat_segment(1))
    ctx.profile_enable(False)
    stages = {s: round(ctx.profile_read(s)[1], 2) for s in SCOPES}
    return {"flat_build_ms": build_ms, "write_flat_ms": write_ms, "stages_ms": {k: v for k, v in stages.items() if v}}, img


def old_path(kind):
    t = {}
    cent, t["kmeans_train_ms"] = wall(lambda: vg.kmeans_train(ctx, base, dim, parts, 0, 10, seed))
    assign, t["kmeans_assign_ms"] = wall(lambda: vg.kmeans_assign(ctx, base, cent, dim, 0))

    def regroup():
        order = torch.argsort(assign.long(), stable=True)
        return order, base[order]
    (order, x), t["argsort_gather_ms"] = wall(regroup)
    off = torch.searchsorted(assign[order].contiguous(), torch.arange(parts + 1, device="cuda", dtype=torch.int32)).cpu().numpy().astype(np.uint32)
    idx = vg.Index(ctx, n, dim)
    _, t["set_vectors_partitions_ms"] = wall(lambda: (idx.set_vectors(x), idx.set_partitions(cent.cpu().numpy(), off)))
    q, codes = quantizer(kind), None
    if kind == "sq8":
        codes, t["quantize_ms"] = wall(lambda: (q.train(x), q.encode(x))[1])
        idx.set_sq8_codes(q, codes)
    elif kind == "pq":
        codes, t["quantize_ms"] = wall(lambda: (q.train(x, 20, seed), q.encode(x))[1])
        idx.set_pq_codes(q, codes)

    def host_image():
        kw = {}
        if kind == "sq8":
            kw.update(quant=ref.QUANT_SQ8, sq_mins=q.params()[0], sq_maxs=q.params()[1], codes=codes.cpu().numpy())
        if kind == "pq":
            cb, sc, of = q.codebooks()
            kw.update(quant=ref.QUANT_PQ, pq_m=m, pq_scales=sc, pq_offsets=of, pq_codebooks=cb, codes=codes.cpu().numpy())
        return ref.image(1, x.cpu().numpy(), dim, 0, centroids=cent.cpu().numpy(), part_offsets=off, checksum=vg.crc32c, **kw)
    img, t["host_image_ms"] = wall(host_image)
    t["total_ms"] = round(sum(t.values()), 1)
    return t, img


out = {"rows": n, "dim": dim, "partitions": parts}
new_path("none")  # warm-up: code objects, scratch blocks
for kind in ("none", "sq8", "pq"):
    new, img_new = new_path(kind)
    old, img_old = old_path(kind)
    new["total_ms"] = round(new["flat_build_ms"] + new["write_flat_ms"], 1)
    out[kind] = {"new": new, "old": old, "same_image": img_new == img_old, "image_bytes": len(img_new)}
    del img_new, img_old
host = base.cpu().numpy()
_, dev_ms = wall(lambda: vg.crc32c_device(ctx, base))
t0 = time.perf_counter()
vg.crc32c(host)
host_ms = round((time.perf_counter() - t0) * 1e3, 1)
out["crc32c"] = {"bytes": host.nbytes, "device_ms": dev_ms, "host_ms": host_ms, "device_gbps": round(host.nbytes / 1e6 / dev_ms, 1),
                 "host_gbps": round(host.nbytes / 1e6 / host_ms, 2)}
print(json.dumps(out))
