"""vg_flat_build, vg_segment_write_flat and vg_crc32c_device on the GPU against flat.Writer.Flush restated in numpy
(tests/flat_writer_ref.py) and against the library's own separate calls: every comparison is exact."""
import ctypes as C
import signal
import time

import numpy as np
import pytest

from tests import flat_writer_ref as ref
from tests import segfile

pytestmark = pytest.mark.gpu

F32, PQ, SQ8 = 0, 1, 2   # VG_SCAN_*


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def rows_for(kind, rng, n, dim):
    if kind == "skewed":          # nine rows in ten in one tight blob
        x = rng.standard_normal((n, dim)).astype(np.float32)
        blob = rng.random(n) < 0.9
        x[blob] = (x[blob] * 0.01 + 3.0).astype(np.float32)
        return x
    if kind == "few points":      # 5 distinct rows: centroids repeat, ties go to the lower partition, the others stay empty
        pts = rng.standard_normal((5, dim)).astype(np.float32)
        return pts[rng.integers(0, 5, n)]
    return rng.standard_normal((n, dim)).astype(np.float32)


def composition(vg, ctx, base, dim, metric, parts, seed):
    """centroids, assignments and the helper's grouping from the separate calls"""
    cent = vg.kmeans_train(ctx, base, dim, parts, metric, 10, seed)
    assign = vg.kmeans_assign(ctx, base, cent, dim, metric)
    return (cent,) + ref.group(assign, parts)


@pytest.mark.parametrize("n,dim,parts,metric,kind", [(3001, 32, 2, 0, "random"), (5003, 24, 7, 1, "random"), (20011, 16, 122, 2, "random"),
                                                     (30001, 8, 1000, 0, "random"), (40003, 8, 5000, 0, "random"),
                                                     (10007, 16, 7, 0, "skewed"), (4099, 16, 7, 0, "few points"),
                                                     (2049, 16, 7, 2, "few points")])
def test_grouping_is_the_writers(vg, ctx, n, dim, parts, metric, kind):
    rng = np.random.default_rng(n + parts)
    base = rows_for(kind, rng, n, dim)
    cent, perm, inv, off = composition(vg, ctx, base, dim, metric, parts, seed=n)
    if kind == "few points":
        assert np.any(np.diff(off.astype(np.int64)) == 0), "the case is meant to leave partitions empty"
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    gperm, ginv = idx.flat_build(parts, seed=n)
    assert np.array_equal(gperm, perm)
    assert np.array_equal(ginv, inv)
    img = idx.write_flat_segment(5)
    h = ref.parse_header(img)
    assert h["num_partitions"] == parts
    got_off = np.frombuffer(img, "<u4", parts + 1, h["part_off_off"])
    assert np.array_equal(got_off, off)
    assert np.array_equal(bits(np.frombuffer(img, "<f4", parts * dim, h["centroid_off"])), bits(cent.ravel()))
    # the index's rows are base[perm]: the image's row section is read from them
    assert img[h["vector_off"]:h["pk_off"]] == base[perm].tobytes()
    assert img == ref.image(5, base[perm], dim, metric, centroids=cent, part_offsets=off, checksum=segfile.crc32c_py if n < 6000 else vg.crc32c)


def by_hand(vg, ctx, base, dim, metric, parts, seed, quant, m, bf16):
    cent, perm, inv, off = composition(vg, ctx, base, dim, metric, parts, seed)
    x = np.ascontiguousarray(base[perm])
    idx = vg.Index(ctx, x.shape[0], dim, vg.Metric(metric))
    idx.set_vectors(x)
    if bf16:
        idx.enable_bf16_filter(True)
    idx.set_partitions(cent, off)
    q, codes = None, None
    if quant == "sq8":
        q = vg.ScalarQuantizer(ctx, dim)
        q.train(x)
        codes = q.encode(x)
        idx.set_sq8_codes(q, codes)
    elif quant == "pq":
        q = vg.ProductQuantizer(ctx, dim, m, 256)
        q.train(x, 20, seed)
        codes = q.encode(x)
        idx.set_pq_codes(q, codes)
    return idx, q, codes, cent, perm, off, x


@pytest.mark.parametrize("quant,metric,parts,bf16", [("none", 0, 7, False), ("none", 2, 40, True), ("sq8", 0, 7, False), ("sq8", 1, 40, True),
                                                     ("pq", 0, 7, True), ("pq", 0, 40, False)])
def test_build_equals_the_separate_calls(vg, ctx, quant, metric, parts, bf16):
    n, dim, m, seed = 6001, 64, 8, 17
    rng = np.random.default_rng(parts + metric)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((12, dim)).astype(np.float32)
    want, wq, wcodes, cent, perm, off, x = by_hand(vg, ctx, base, dim, metric, parts, seed, quant, m, bf16)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    if bf16:
        idx.enable_bf16_filter(True)   # before the build: its image is permuted with the rows
    gq = {"none": None, "sq8": vg.ScalarQuantizer(ctx, dim), "pq": vg.ProductQuantizer(ctx, dim, m, 256)}[quant]
    gperm, _ = idx.flat_build(parts, gq, seed=seed)
    assert np.array_equal(gperm, perm)
    img = idx.write_flat_segment(1)
    h = ref.parse_header(img)
    if quant == "sq8":
        for a, b in zip(gq.params(), wq.params()):
            assert np.array_equal(bits(a), bits(b))
        assert img[h["codes_off"]:h["vector_off"]] == wcodes.tobytes()
    if quant == "pq":
        (cb, sc, of), (wcb, wsc, wof) = gq.codebooks(), wq.codebooks()
        assert np.array_equal(cb, wcb) and np.array_equal(bits(sc), bits(wsc)) and np.array_equal(bits(of), bits(wof))
        assert img[h["codes_off"]:h["vector_off"]] == wcodes.tobytes()
    scans = [F32] + ([SQ8] if quant == "sq8" else []) + ([PQ] if quant == "pq" else [])
    for scan in scans:
        for nprobes in (1, 8, parts):
            gi, gs = idx.search_flat_probed(queries, 10, nprobes, scan)
            wi, ws = want.search_flat_probed(queries, 10, nprobes, scan)
            assert np.array_equal(gi, wi), (scan, nprobes)
            assert np.array_equal(bits(gs), bits(ws)), (scan, nprobes)


def test_skip_rules(vg, ctx):
    rng = np.random.default_rng(3)
    dim = 16
    for n, parts in ((5, 8), (100, 1), (100, 0)):
        base = rng.standard_normal((n, dim)).astype(np.float32)
        idx = vg.Index(ctx, n, dim)
        idx.set_vectors(base)
        sq = vg.ScalarQuantizer(ctx, dim)
        perm, inv = idx.flat_build(parts, sq)
        assert np.array_equal(perm, np.arange(n)) and np.array_equal(inv, np.arange(n))
        img = idx.write_flat_segment(2)
        h = ref.parse_header(img)
        assert h["num_partitions"] == 0 and h["part_off_off"] == h["centroid_off"] == ref.HEADER_SIZE and h["quant"] == ref.QUANT_SQ8
        want = vg.ScalarQuantizer(ctx, dim)
        want.train(base)
        assert img == ref.image(2, base, dim, 0, quant=ref.QUANT_SQ8, sq_mins=want.params()[0], sq_maxs=want.params()[1], codes=want.encode(base))
    empty = vg.Index(ctx, 0, dim)
    assert empty.flat_build(4)[0].size == 0
    assert empty.write_flat_segment(9) == ref.image(9, np.zeros((0, dim), np.float32), dim, 0)


def test_refusals_change_nothing(vg, ctx):
    rng = np.random.default_rng(4)
    n, dim = 900, 16
    base = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((4, dim)).astype(np.float32)
    lib = ctx._lib

    def status(idx, parts=4, kind=0, pq_m=0, sq=None, pq=None, perm=None):
        return lib.vg_flat_build(idx._h, C.c_int32(parts), C.c_int32(kind), C.c_int32(pq_m), C.c_int32(0), C.c_int32(0), C.c_uint64(1),
                                 sq._h if sq else None, pq._h if pq else None, None if perm is None else C.c_void_p(perm.ctypes.data), None,
                                 None)

    def fresh(metric=0):
        idx = vg.Index(ctx, n, dim, vg.Metric(metric))
        idx.set_vectors(base)
        return idx

    assert status(vg.Index(ctx, n, dim)) == -9                      # no fp32 rows: VG_ERR_NOT_READY
    assert status(vg.Index(ctx, n, dim, vg.Metric.HAMMING)) in (-9, -5)
    ham = vg.Index(ctx, 0, dim, vg.Metric.HAMMING)
    assert status(ham) == -5                                        # Hamming: VG_ERR_UNSUPPORTED
    sq = vg.ScalarQuantizer(ctx, dim)
    sq.train(base)
    pq = vg.ProductQuantizer(ctx, dim, 4, 256)
    cases = []
    g = fresh()
    g.build_hnsw(m=8, ef_construction=32, max_batch=64, growth_div=16)
    cases.append(("hnsw", g, lambda i: i.search_hnsw(queries, 5, 32)))
    v = fresh()
    v.build_vamana(r=8, l=16)
    cases.append(("vamana", v, lambda i: i.search_vamana(queries, 5, 0)))
    c = fresh()
    c.set_sq8_codes(sq, sq.encode(base))
    cases.append(("codes", c, lambda i: i.search_sq8(queries, 5)))
    p = fresh()
    p.set_partitions(base[:2], np.array([0, 400, n], np.uint32))
    cases.append(("partitions", p, lambda i: i.search_flat_probed(queries, 5, 1, F32)))
    for name, idx, search in cases:
        before = search(idx)
        perm = np.full(n, 7, np.uint32)
        assert status(idx, perm=perm) == -5, name                   # VG_ERR_UNSUPPORTED
        assert np.all(perm == 7), name
        after = search(idx)
        assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1])), name
    idx = fresh()
    before = idx.search_flat(queries, 5)
    assert status(idx, kind=3) == -1                                # SQ8 without its quantizer
    assert status(idx, kind=1) == -1                                # PQ without its quantizer
    assert status(idx, kind=2) == -1                                # not a flat quantization type
    assert status(idx, kind=3, sq=vg.ScalarQuantizer(ctx, dim + 1)) == -2
    assert status(idx, kind=1, pq=vg.ProductQuantizer(ctx, dim * 2, 4, 256)) == -2
    assert status(idx, kind=1, pq_m=8, pq=pq) == -1                 # the vg_pq is (dim, 4), the call says 8
    wide = vg.Index(ctx, 10, 600)
    wide.set_vectors(rng.standard_normal((10, 600)).astype(np.float32))
    assert status(wide, parts=0, kind=1, pq_m=2, pq=vg.ProductQuantizer(ctx, 600, 2, 256)) == -5   # sub-vector dim 300: vg_pq_train's refusal
    after = idx.search_flat(queries, 5)
    assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1]))
    # the image writer's refusals
    buf = np.zeros(64, np.uint8)
    assert lib.vg_segment_write_flat(idx._h, C.c_uint64(1), None, None, C.c_int64(0), None, C.c_int64(0), C.c_void_p(buf.ctypes.data),
                                     C.c_int64(buf.size), None, None) == -1 and not buf.any()
    assert lib.vg_segment_write_flat(idx._h, C.c_uint64(1), None, None, C.c_int64(0), None, C.c_int64(0), None, C.c_int64(1 << 30), None,
                                     None) == -1
    lib.vg_segment_flat_image_size.restype = C.c_int64
    assert lib.vg_segment_flat_image_size(vg.Index(ctx, n, dim)._h, C.c_int64(-1), C.c_int64(-1)) == -1     # rows > 0, none attached
    assert lib.vg_segment_flat_image_size(g._h, C.c_int64(-1), C.c_int64(-1)) == -1                         # a graph
    r = fresh()
    r.set_rabitq_codes(vg.RaBitQuantizer(ctx, dim).encode(base))
    assert lib.vg_segment_flat_image_size(r._h, C.c_int64(-1), C.c_int64(-1)) == -1                         # RaBitQ codes


def test_crc32c_device(vg, ctx):
    import torch
    rng = np.random.default_rng(5)
    chunk = 256 * 1024            # the bytes one workgroup covers
    host = rng.integers(0, 256, 3 * chunk + 4096, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    for size in (0, 1, 7, 8, 9, 15, 16, 17, 4095, chunk - 1, chunk, chunk + 1, 2 * chunk + 33):
        for start in range(16):
            got = vg.crc32c_device(ctx, dev[start:start + size])
            assert got == vg.crc32c(host[start:start + size].tobytes()), (size, start)
            if size <= 4095:
                assert got == segfile.crc32c_py(host[start:start + size].tobytes()), (size, start)
    big = rng.integers(0, 256, 100_000_003, dtype=np.uint8)
    dbig = torch.from_numpy(big).cuda()
    for start in (0, 5):
        assert vg.crc32c_device(ctx, dbig[start:]) == vg.crc32c(big[start:])
    with pytest.raises(TypeError):
        vg.crc32c_device(ctx, torch.from_numpy(host))


@pytest.mark.parametrize("quant", ["none", "sq8", "pq"])
@pytest.mark.parametrize("parts", [0, 9])
@pytest.mark.parametrize("docs", [False, True])
def test_image_is_the_writers(vg, ctx, quant, parts, docs):
    n, dim, m, seed, metric = 4100, 40, 5, 23, 0          # 4100 rows: 5 blocks of statistics; odd section sizes: nothing is aligned
    rng = np.random.default_rng(parts + len(quant))
    base = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((8, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    gq = {"none": None, "sq8": vg.ScalarQuantizer(ctx, dim), "pq": vg.ProductQuantizer(ctx, dim, m, 256)}[quant]
    perm, _ = idx.flat_build(parts, gq, seed=seed)
    x = base[perm]
    kw = {}
    if parts:
        cent, wperm, _, off = composition(vg, ctx, base, dim, metric, parts, seed)
        assert np.array_equal(perm, wperm)
        kw.update(centroids=cent, part_offsets=off)
    if quant == "sq8":
        w = vg.ScalarQuantizer(ctx, dim)
        w.train(x)
        kw.update(quant=ref.QUANT_SQ8, sq_mins=w.params()[0], sq_maxs=w.params()[1], codes=w.encode(x))
    if quant == "pq":
        w = vg.ProductQuantizer(ctx, dim, m, 256)
        w.train(x, 20, seed)
        cb, sc, of = w.codebooks()
        kw.update(quant=ref.QUANT_PQ, pq_m=m, pq_scales=sc, pq_offsets=of, pq_codebooks=cb, codes=w.encode(x))
    ids = md = bs = None
    if docs:   # what the host passes: its ids and its serialised documents, permuted like the rows
        ids = (rng.integers(0, 1 << 62, n, dtype=np.uint64))[perm]
        lens = rng.integers(0, 4, n)
        md = np.concatenate([[0], np.cumsum(lens)]).astype("<u4").tobytes() + bytes(rng.integers(0, 256, int(lens.sum()), dtype=np.uint8))
        bs = ref.uvarint(5) + b"".join(ref.uvarint(3) + b"\x01\x01a"[:3] for _ in range(5))
    img = idx.write_flat_segment(0xABCDEF0123, ids, md, bs)
    want = ref.image(0xABCDEF0123, x, dim, metric, ids=ids, metadata=md, block_stats=bs, checksum=vg.crc32c, **kw)
    assert len(img) == len(want)
    assert img == want
    lib = ctx._lib
    lib.vg_segment_flat_image_size.restype = C.c_int64
    assert lib.vg_segment_flat_image_size(idx._h, C.c_int64(-1 if md is None else len(md)), C.c_int64(-1 if bs is None else len(bs))) == len(want)
    assert ref.parse_header(img)["checksum"] == segfile.crc32c_py(img[ref.HEADER_SIZE:])
    # the reader takes the reference writer's own, unpadded layout
    seg = vg.Segment(ctx, img, "flat", verify_checksum=True)
    info = seg.info
    assert (info.segment_id, info.rows, info.dim, info.metric, info.kind, info.num_partitions) == (0xABCDEF0123, n, dim, metric, 0, parts)
    assert info.quantization == {"none": 0, "sq8": 3, "pq": 1}[quant]
    scan = {"none": F32, "sq8": SQ8, "pq": PQ}[quant]
    for nprobes in (1, 4):
        si, ss = seg.search(queries, 10, nprobes)
        gi, gs = idx.search_flat_probed(queries, 10, nprobes, scan)
        assert np.array_equal(si, gi) and np.array_equal(bits(ss), bits(gs)), nprobes


FULL_SIZE_LIMIT_S = 600   # the whole test; see its docstring


def test_full_size(vg, ctx):
    """1M x 768, 122 partitions, SQ8: the order against torch's stable argsort, the image's checksum against the host CRC, the
    image opened and searched.  Time limit: FULL_SIZE_LIMIT_S for the whole test, from its parts' known costs rather than a
    measured run: ten k-means iterations twice (here and inside the build) at about a second each at this size at worst,
    3.8 GB over the bus once per image, a host CRC of 3.8 GB at 1 GB/s or better, two 1M-element sorts — under a minute; the
    limit leaves an order of magnitude for a busy host.  The test prints its stage times."""
    import torch

    def too_long(*_):
        raise TimeoutError(f"test_full_size ran past {FULL_SIZE_LIMIT_S} s")
    old = signal.signal(signal.SIGALRM, too_long)
    signal.alarm(FULL_SIZE_LIMIT_S)
    try:
        n, dim, parts, seed = 1_000_000, 768, 122, 42
        t0 = time.time()
        g = torch.Generator(device="cuda").manual_seed(7)
        dbase = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
        dbase += 2.0 * torch.randn((64, dim), generator=g, device="cuda")[torch.randint(0, 64, (n,), generator=g, device="cuda")]
        queries = dbase[:64].cpu().numpy() + 0.01
        cent = vg.kmeans_train(ctx, dbase, dim, parts, 0, 10, seed)
        assign = vg.kmeans_assign(ctx, dbase, cent, dim, 0)
        assign = assign if isinstance(assign, torch.Tensor) else torch.from_numpy(np.asarray(assign)).cuda()
        want = torch.argsort(assign.long(), stable=True).cpu().numpy().astype(np.uint32)
        idx = vg.Index(ctx, n, dim)
        idx.set_vectors(dbase)
        del dbase
        sq = vg.ScalarQuantizer(ctx, dim)
        t1 = time.time()
        perm, inv = idx.flat_build(parts, sq, seed=seed)
        t2 = time.time()
        assert np.array_equal(perm, want)
        assert np.array_equal(inv[perm], np.arange(n, dtype=np.uint32))
        img = idx.write_flat_segment(1)
        t3 = time.time()
        h = ref.parse_header(img)
        body = np.frombuffer(img, np.uint8, len(img) - ref.HEADER_SIZE, ref.HEADER_SIZE)
        assert h["checksum"] == vg.crc32c(body)
        t4 = time.time()
        seg = vg.Segment(ctx, img, "flat", verify_checksum=False)
        for nprobes in (1, 8):
            si, ss = seg.search(queries, 10, nprobes)
            gi, gs = idx.search_flat_probed(queries, 10, nprobes, SQ8)
            assert np.array_equal(si, gi) and np.array_equal(bits(ss), bits(gs))
        print(f"full size: setup {t1 - t0:.1f} s, flat_build {t2 - t1:.2f} s, write_flat_segment {t3 - t2:.2f} s, "
              f"host crc of the body {t4 - t3:.2f} s, total {time.time() - t0:.1f} s")
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)
