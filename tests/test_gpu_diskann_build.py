"""vg_diskann_build and vg_segment_write_diskann on the GPU against diskann.Writer.Flush restated in numpy
(tests/diskann_writer_ref.py) and against the library's own separate calls: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from tests import diskann_writer_ref as ref
from tests import reorder_bfs_ref, segfile, vamana_build_ref

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_DIM_MISMATCH, ERR_UNSUPPORTED, ERR_NOT_READY = -1, -2, -5, -9
NONE, PQ, SQ8, RABITQ, INT4 = 0, 1, 3, 5, 6          # VG_QUANT_*
WALK = {NONE: 0, PQ: 1, RABITQ: 2, INT4: 3}          # vg_search_vamana's kind for a segment of that quantization
KINDS = ("none", "pq", "rabitq", "int4")


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def hand_graph(rng, n, r):
    """random lists without self edges, some rows with empty slots in the middle, row 1 empty"""
    g = np.empty((n, r), np.uint32)
    for i in range(n):
        g[i] = rng.choice(np.delete(np.arange(n), i), r, replace=False)
    g[rng.integers(0, n, n // 4), rng.integers(1, r - 1, n // 4)] = ref.EMPTY
    g[1] = ref.EMPTY
    return g


def attach(vg, ctx, idx, kind, x, pq_m, rng):
    """codes of `kind` attached by the separate calls; returns (the helper's keyword arguments, what keeps the quantizer alive)"""
    dim = x.shape[1]
    if kind == "pq":       # 37 rows cannot train 256 centroids: codebooks set by hand, as a segment file would bring them
        q = vg.ProductQuantizer(ctx, dim, pq_m, 256)
        q.set_codebooks(rng.integers(-128, 128, pq_m * 256 * (dim // pq_m), dtype=np.int8), rng.random(pq_m).astype(np.float32) + 0.5,
                        rng.standard_normal(pq_m).astype(np.float32))
        codes = q.encode(x)
        idx.set_pq_codes(q, codes)
        cb, sc, of = q.codebooks()
        return dict(quant=ref.QUANT_PQ, pq_m=pq_m, codes=codes, pq_scales=sc, pq_offsets=of, pq_codebooks=cb), q
    if kind == "rabitq":
        codes = vg.RaBitQuantizer(ctx, dim).encode(x)
        idx.set_rabitq_codes(codes)
        return dict(quant=ref.QUANT_RABITQ, codes=codes), None
    if kind == "int4":
        q = vg.Int4Quantizer(ctx, dim)
        q.train(x)
        codes = q.encode(x)
        idx.set_int4_codes(q, codes)
        mn, df, _ = q.params()
        return dict(quant=ref.QUANT_INT4, codes=codes, int4_min=mn, int4_diff=df), q
    return {}, None


def size_of(ctx, idx, md=None, mi=None):
    ctx._lib.vg_segment_diskann_image_size.restype = C.c_int64
    return ctx._lib.vg_segment_diskann_image_size(idx._h, C.c_int64(-1 if md is None else len(md)), C.c_int64(-1 if mi is None else len(mi)))


# ---- 1 + 3: the image's bytes, and the reader takes them -----------------------------------------------------------------
@pytest.mark.parametrize("kind,dim", [(k, 12) for k in KINDS] + [("int4", 7), ("rabitq", 7)])
@pytest.mark.parametrize("docs,compression", [(True, 1), (False, 0)])
def test_image_is_the_writers_and_opens(vg, ctx, kind, dim, docs, compression):
    n, r, m, entry, metric = 37, 5, 3, 11, 0          # PQ: 111 code bytes; dim 7: 4 INT4 bytes of 3.5, nothing 8-aligned
    rng = np.random.default_rng(dim + len(kind))
    x = rng.standard_normal((n, dim)).astype(np.float32)
    g = hand_graph(rng, n, r)
    queries = rng.standard_normal((6, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(x)
    idx.set_vamana_graph(g, entry)
    kw, keep = attach(vg, ctx, idx, kind, x, m, rng)
    ids = md = mi = None
    if docs:       # ids beyond 2^32, both metadata sections with odd lengths
        ids = rng.integers(1 << 33, 1 << 62, n, dtype=np.uint64)
        lens = rng.integers(0, 4, n)
        lens[0] += (int(lens.sum()) + 1) % 2          # an odd blob behind the 8 * (n + 1) offset bytes
        md = np.concatenate([[0], np.cumsum(lens)]).astype("<u8").tobytes() + bytes(rng.integers(0, 256, int(lens.sum()), dtype=np.uint8))
        mi = b"\x02\x03tag\x01\x05"
        assert len(md) % 2 == 1 and len(mi) % 2 == 1
    img = idx.write_diskann_segment(0xABCDEF0123, 64 if docs else 0, compression, ids, md, mi)
    want = ref.image(0xABCDEF0123, x, dim, metric, g, entry, search_list=64 if docs else 100, compression=compression, ids=ids,
                     metadata=md, metadata_index=mi, checksum=segfile.crc32c_py, **kw)
    assert len(img) == len(want) == size_of(ctx, idx, md, mi)
    assert img == want
    h = ref.parse_header(img)
    assert h["checksum"] == segfile.crc32c_py(img[ref.HEADER_SIZE:])
    # written, through the C call: the image size, also into a larger buffer whose rest stays untouched
    buf = np.full(len(want) + 9, 0xEE, np.uint8)
    written = C.c_int64(-1)
    amd = None if md is None else np.frombuffer(md, np.uint8)
    ami = None if mi is None else np.frombuffer(mi, np.uint8)
    st = ctx._lib.vg_segment_write_diskann(idx._h, C.c_uint64(0xABCDEF0123), C.c_int32(64 if docs else 0), C.c_int32(compression),
                                           None if ids is None else C.c_void_p(ids.ctypes.data),
                                           None if md is None else C.c_void_p(amd.ctypes.data), C.c_int64(len(md) if docs else 0),
                                           None if mi is None else C.c_void_p(ami.ctypes.data), C.c_int64(len(mi) if docs else 0),
                                           C.c_void_p(buf.ctypes.data), C.c_int64(buf.size), C.byref(written), None)
    assert st == 0 and written.value == len(want) and np.all(buf[len(want):] == 0xEE)
    assert buf[:len(want)].tobytes() == want
    # the reader takes the reference writer's own layout: unpadded, odd-sized code sections, non-zero metadata offsets
    seg = vg.Segment(ctx, img, "diskann", verify_checksum=True)
    info = seg.info
    quant = kw.get("quant", NONE)
    assert (info.segment_id, info.rows, info.dim, info.metric, info.kind) == (0xABCDEF0123, n, dim, metric, 1)
    assert (info.quantization, info.max_degree, info.search_list_size, info.entrypoint) == (quant, r, 64 if docs else 100, entry)
    assert (info.pq_m, info.pq_k) == ((m, 256) if kind == "pq" else (0, 0))
    si, ss = seg.search(queries, 5)
    gi, gs = idx.search_vamana(queries, 5, WALK[quant])
    assert np.array_equal(si, gi) and np.array_equal(bits(ss), bits(gs))
    mask = rng.random(n) < 0.5
    si, ss = seg.search_filtered(queries, 5, mask)
    gi, gs = idx.search_vamana_filtered(queries, 5, mask, WALK[quant])
    assert np.array_equal(si, gi) and np.array_equal(bits(ss), bits(gs))
    seg.close()


# ---- 2: the checksum chained over the device CRC kernel's blocks ------------------------------------------------------------
# A block of crc_blocks_kernel covers 256 KiB (kCrcBlockBytes, k_flat_build.hip).  The device sections — rows, graph, codes —
# begin at multiples of 4 inside the body whatever the shape (a 160-byte header, then fp32 and uint32 sections), so the second
# case has them begin and end off the kernel's 16-byte pieces (body offsets 12 and 8 mod 16) instead; device ADDRESSES of every
# alignment are tests/test_gpu_flat_build.py::test_crc32c_device's.
@pytest.mark.parametrize("n,dim,r,kind", [(3000, 64, 5, "none"), (3001, 63, 3, "int4")])
def test_checksum_chains_over_blocks(vg, ctx, n, dim, r, kind):
    assert n * dim * 4 > 2 * 256 * 1024               # the rows span three blocks
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    g = rng.integers(0, n, (n, r)).astype(np.uint32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(x)
    idx.set_vamana_graph(g, 0)
    kw, keep = attach(vg, ctx, idx, kind, x, 0, rng)
    img = idx.write_diskann_segment(3)
    h = ref.parse_header(img)
    if kind == "int4":
        assert (h["graph_off"] - ref.HEADER_SIZE) % 16 == 12 and (h["pq_codes_off"] - ref.HEADER_SIZE) % 16 == 8
    assert h["checksum"] == segfile.crc32c_py(img[ref.HEADER_SIZE:])
    assert img == ref.image(3, x, dim, 0, g, 0, checksum=vg.crc32c, **kw)


# ---- 4: build = the three groups of calls, one after another ----------------------------------------------------------------
def quantizer_for(vg, ctx, kind, dim, m):
    return {"none": None, "pq": vg.ProductQuantizer(ctx, dim, m, 256) if kind == "pq" else None,
            "rabitq": vg.RaBitQuantizer(ctx, dim), "int4": vg.Int4Quantizer(ctx, dim) if kind == "int4" else None}[kind]


def by_hand(vg, ctx, base, metric, kind, m, r, l, seed, max_batch):
    n, dim = base.shape
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    q = quantizer_for(vg, ctx, kind, dim, m)
    if kind == "pq":
        q.train(base, 20, seed)
        idx.set_pq_codes(q, q.encode(base))
    elif kind == "rabitq":
        idx.set_rabitq_codes(q.encode(base))
    elif kind == "int4":
        q.train(base)
        idx.set_int4_codes(q, q.encode(base))
    idx.build_vamana(r=r, l=l, alpha=1.2, seed=seed, max_batch=max_batch, growth_div=32)
    perm, inv = idx.reorder_vamana_bfs()
    return idx, q, perm, inv


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("max_batch", [1, 64])
def test_build_equals_the_separate_calls(vg, ctx, kind, metric, max_batch):
    n, dim, m, r, l, seed = 300, 16, 4, 8, 20, 17
    rng = np.random.default_rng(metric + len(kind))
    base = rng.standard_normal((n, dim)).astype(np.float32)
    want, wq, wperm, winv = by_hand(vg, ctx, base, metric, kind, m, r, l, seed, max_batch)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    gq = quantizer_for(vg, ctx, kind, dim, m)
    perm, inv, used = idx.diskann_build(r, l, 1.2, gq, seed=seed, max_batch=max_batch, growth_div=32)
    assert used == {"none": NONE, "pq": PQ, "rabitq": RABITQ, "int4": INT4}[kind]
    assert np.array_equal(perm, wperm) and np.array_equal(inv, winv)
    assert np.array_equal(inv[perm], np.arange(n, dtype=np.uint32))
    (g, entry), (wg, wentry) = idx.get_vamana_graph(), want.get_vamana_graph()
    assert entry == wentry == 0 and np.array_equal(g, wg)
    ids = (np.arange(n, dtype=np.uint64) + (1 << 35))[perm]
    a, b = idx.write_diskann_segment(5, l, 1, ids), want.write_diskann_segment(5, l, 1, ids)
    assert a == b
    h = ref.parse_header(a)
    assert h["quant"] == used and img_rows(a, h, n, dim) == base[perm].tobytes()


def img_rows(img, h, n, dim):
    return img[h["vector_off"]:h["vector_off"] + n * dim * 4]


def test_build_against_the_restated_writer(vg, ctx):
    """n = 120, max_batch = 1: graph and permutation against buildGraph and reorderBFS restated in Python"""
    n, dim, r, l, seed = 120, 16, 8, 20, 9
    base = np.random.default_rng(1).standard_normal((n, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    perm, inv, used = idx.diskann_build(r, l, 1.2, None, seed=seed, max_batch=1)
    eg, eentry = vamana_build_ref.build(base, 0, r, l, 1.2, seed=seed, max_batch=1)
    eperm, einv, ng, nentry = reorder_bfs_ref.reorder(eg, eentry)
    g, entry = idx.get_vamana_graph()
    assert used == NONE and entry == nentry
    assert np.array_equal(perm, eperm) and np.array_equal(inv, einv) and np.array_equal(g, ng)
    assert idx.write_diskann_segment(1, l) == ref.image(1, base[perm], dim, 0, ng, nentry, search_list=l, checksum=segfile.crc32c_py)


# ---- 5: trainPQ's rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,trains", [(200, False), (256, True)])
def test_train_pq_rule(vg, ctx, n, trains):
    dim, m = 16, 4
    base = np.random.default_rng(n).standard_normal((n, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    pq = vg.ProductQuantizer(ctx, dim, m, 256)
    perm, inv, used = idx.diskann_build(8, 20, 1.2, pq, seed=3, max_batch=64)
    h = ref.parse_header(idx.write_diskann_segment(1))
    assert pq.is_trained() == trains and used == (PQ if trains else NONE)
    assert (h["quant"], h["pq_m"], h["pq_k"]) == ((PQ, m, 256) if trains else (NONE, 0, 0))
    assert (h["pq_codes_off"] != 0) == (h["pq_codebook_off"] != 0) == trains and h["bq_codes_off"] == 0
    if trains:
        w = vg.ProductQuantizer(ctx, dim, m, 256)
        w.train(base, 20, 3)
        assert all(np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)) for a, b in zip(pq.codebooks(), w.codebooks()))
    else:       # no codes: the walk over PQ codes has nothing to read
        with pytest.raises(vg.VecgoHipError):
            idx.search_vamana(base[:2], 3, 1)


# ---- 6: refusals, in the documented order, change nothing ----------------------------------------------------------------------
def test_build_refusals_change_nothing(vg, ctx):
    rng = np.random.default_rng(4)
    n, dim = 300, 16
    base = rng.standard_normal((n, dim)).astype(np.float32)
    queries = rng.standard_normal((4, dim)).astype(np.float32)
    lib = ctx._lib
    perm = np.full(n, 7, np.uint32)
    used = C.c_int32(77)

    def status(idx, kind=NONE, pq_m=0, pq=None, iq=None, r=8, l=20, max_batch=64, growth_div=32, pq_iters=0):
        st = lib.vg_diskann_build(idx._h, C.c_int32(r), C.c_int32(l), C.c_float(1.2), C.c_int32(kind), C.c_int32(pq_m), C.c_int32(pq_iters),
                                  C.c_uint64(1), C.c_int32(max_batch), C.c_int32(growth_div), pq._h if pq else None, iq._h if iq else None,
                                  C.c_void_p(perm.ctypes.data), C.c_void_p(perm.ctypes.data), C.byref(used), None)
        assert np.all(perm == 7) and used.value == 77
        return st

    def fresh():
        idx = vg.Index(ctx, n, dim)
        idx.set_vectors(base)
        return idx

    pq4 = vg.ProductQuantizer(ctx, dim, 4, 256)
    # 2, 3: no fp32 rows before everything about the arguments; no rows
    assert status(vg.Index(ctx, n, dim), kind=2) == ERR_NOT_READY
    assert status(vg.Index(ctx, 0, dim)) == ERR_INVALID_ARG and b"no vectors to write" in lib.vg_last_error()
    # 4: state the writer never starts from, before the arguments (kind 2 is unknown)
    trained = vg.ProductQuantizer(ctx, dim, 4, 256)
    trained.train(base, 2, 1)
    iq = vg.Int4Quantizer(ctx, dim)
    iq.train(base)
    held = []
    a = fresh(); a.set_pq_codes(trained, trained.encode(base)); held.append(("pq codes", a, lambda i: i.search_pq_adc(queries, 5)))
    a = fresh(); a.set_int4_codes(iq, iq.encode(base)); held.append(("int4 codes", a, lambda i: i.search_flat(queries, 5)))
    a = fresh(); a.set_rabitq_codes(vg.RaBitQuantizer(ctx, dim).encode(base)); held.append(("rabitq codes", a, lambda i: i.search_rabitq(queries, 5)))
    a = fresh(); a.set_partitions(base[:2], np.array([0, 100, n], np.uint32)); held.append(("partitions", a, lambda i: i.search_flat_probed(queries, 5, 1, 0)))
    a = fresh(); a.build_vamana(r=8, l=16); held.append(("vamana", a, lambda i: i.search_vamana(queries, 5, 0)))
    a = fresh(); a.build_hnsw(m=8, ef_construction=32, max_batch=64, growth_div=16); held.append(("hnsw", a, lambda i: i.search_hnsw(queries, 5, 32)))
    for name, idx, search in held:
        before = search(idx)
        assert status(idx, kind=2) == ERR_UNSUPPORTED, name
        after = search(idx)
        assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1])), name
    # 5 - 9 on one index, which must come out of them bare
    idx = fresh()
    for kind in (2, 4, 7, -1, SQ8):
        assert status(idx, kind=kind, pq_m=4, pq=pq4, iq=iq) == ERR_INVALID_ARG, kind          # 5: unknown kinds, SQ8
    assert status(idx, kind=PQ, pq_m=4) == ERR_INVALID_ARG                                    # 5: PQ without its quantizer
    assert status(idx, kind=INT4) == ERR_INVALID_ARG                                          # 5: INT4 without its quantizer
    assert status(idx, kind=PQ, pq_m=0, pq=pq4) == ERR_INVALID_ARG                            # 6
    assert status(idx, kind=PQ, pq_m=-4, pq=pq4) == ERR_INVALID_ARG
    assert status(idx, kind=PQ, pq_m=8, pq=pq4) == ERR_INVALID_ARG                            # 7: the vg_pq is (dim, 4)
    assert status(idx, kind=PQ, pq_m=2, pq=vg.ProductQuantizer(ctx, dim, 2, 16)) == ERR_INVALID_ARG   # 7: 16 centroids
    assert status(idx, kind=PQ, pq_m=8, pq=vg.ProductQuantizer(ctx, dim * 2, 4, 256)) == ERR_INVALID_ARG   # 7 before 8
    assert status(idx, kind=PQ, pq_m=4, pq=vg.ProductQuantizer(ctx, dim * 2, 4, 256), r=65) == ERR_DIM_MISMATCH   # 8 before 9
    assert status(idx, kind=INT4, iq=vg.Int4Quantizer(ctx, dim + 1), r=65) == ERR_DIM_MISMATCH
    assert status(idx, kind=PQ, pq_m=4, pq=pq4, pq_iters=-1) == ERR_INVALID_ARG               # 9: vg_pq_train's
    wide = vg.Index(ctx, 256, 600)
    wide.set_vectors(rng.standard_normal((256, 600)).astype(np.float32))
    assert status(wide, kind=PQ, pq_m=2, pq=vg.ProductQuantizer(ctx, 600, 2, 256)) == ERR_UNSUPPORTED and b"vg_pq_train" in lib.vg_last_error()
    for bad, want in ((dict(r=65), ERR_UNSUPPORTED), (dict(l=1025), ERR_UNSUPPORTED), (dict(max_batch=0), ERR_INVALID_ARG),
                      (dict(growth_div=0), ERR_INVALID_ARG), (dict(max_batch=16385), ERR_UNSUPPORTED)):
        assert status(idx, kind=PQ, pq_m=4, pq=pq4, **bad) == want, bad                       # 9: vg_vamana_build's, and no codes left
        assert b"vg_vamana_build" in lib.vg_last_error()
        assert status(idx, kind=RABITQ, **bad) == want and status(idx, kind=INT4, iq=vg.Int4Quantizer(ctx, dim), **bad) == want, bad
    assert not pq4.is_trained()
    assert size_of(ctx, idx) == -1                                                            # still no graph
    with pytest.raises(vg.VecgoHipError):
        idx.search_vamana(queries, 3, 1)                                                      # and no codes
    # the refused index builds like a fresh one
    other = fresh()
    assert all(np.array_equal(x, y) for x, y in zip(idx.diskann_build(8, 20, seed=2)[:2], other.diskann_build(8, 20, seed=2)[:2]))
    assert idx.write_diskann_segment(1) == other.write_diskann_segment(1)


def test_write_refusals_write_nothing(vg, ctx):
    rng = np.random.default_rng(6)
    n, dim, r = 60, 8, 4
    base = rng.standard_normal((n, dim)).astype(np.float32)
    g = hand_graph(rng, n, r)
    lib = ctx._lib
    buf = np.full(1 << 16, 0xEE, np.uint8)
    md = np.zeros(16, np.uint8)

    def status(idx, image=buf, size=None, compression=1, search_list=0, md_bytes=None):
        written = C.c_int64(5)
        st = lib.vg_segment_write_diskann(idx._h, C.c_uint64(1), C.c_int32(search_list), C.c_int32(compression), None,
                                          None if md_bytes is None else C.c_void_p(md.ctypes.data), C.c_int64(md_bytes or 0), None, C.c_int64(0),
                                          None if image is None else C.c_void_p(image.ctypes.data),
                                          C.c_int64(buf.size if size is None else size), C.byref(written), None)
        assert np.all(buf == 0xEE) and written.value == 0
        return st

    def fresh(graph=True):
        idx = vg.Index(ctx, n, dim)
        idx.set_vectors(base)
        if graph:
            idx.set_vamana_graph(g, 3)
        return idx

    good = fresh()
    want = good.write_diskann_segment(1)
    nograph = fresh(graph=False)
    # the arguments first, whatever the index holds
    for idx in (good, nograph):
        assert status(idx, image=None) == ERR_INVALID_ARG
        assert status(idx, compression=3) == ERR_INVALID_ARG and status(idx, compression=-1) == ERR_INVALID_ARG
        assert status(idx, search_list=-1) == ERR_INVALID_ARG
        assert status(idx, md_bytes=-1) == ERR_INVALID_ARG
    empty = vg.Index(ctx, 0, dim)
    assert status(empty) == ERR_INVALID_ARG and size_of(ctx, empty) == -1                      # rows == 0
    bare = vg.Index(ctx, n, dim)
    assert status(bare) == ERR_NOT_READY and size_of(ctx, bare) == -1                          # no fp32 rows
    assert status(nograph) == ERR_NOT_READY and size_of(ctx, nograph) == -1                    # no Vamana graph
    sq = vg.ScalarQuantizer(ctx, dim)
    sq.train(base)
    iq = vg.Int4Quantizer(ctx, dim)
    iq.train(base)
    h = fresh(graph=False); h.build_hnsw(m=4, ef_construction=16, max_batch=16, growth_div=8); h.set_vamana_graph(g, 3)
    p = fresh(); p.set_partitions(base[:2], np.array([0, 20, n], np.uint32))
    s = fresh(); s.set_sq8_codes(sq, sq.encode(base))
    two = fresh(); two.set_int4_codes(iq, iq.encode(base)); two.set_rabitq_codes(vg.RaBitQuantizer(ctx, dim).encode(base))
    for name, idx in (("hnsw", h), ("partitions", p), ("sq8", s), ("two kinds of codes", two)):
        assert status(idx) == ERR_UNSUPPORTED, name
        assert size_of(ctx, idx) == -1, name
    # a buffer one byte short, last: everything else about the call is in order
    assert size_of(ctx, good) == len(want)
    assert status(good, size=len(want) - 1) == ERR_INVALID_ARG
    assert status(good, size=-1) == ERR_INVALID_ARG
    assert good.write_diskann_segment(1) == want                                               # the index itself is unchanged
    for c in (0, 1, 2):
        assert ref.parse_header(good.write_diskann_segment(1, 0, c))["compression"] == c
