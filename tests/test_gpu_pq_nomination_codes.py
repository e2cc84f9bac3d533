"""vg_index_enable_pq_nomination_from_codes: the PQ batch nomination WITHOUT the image of the decoded rows.  The nomination GEMM
fills its row tiles from a bfloat16 copy of the decoded codebook by the rows' codes (8 dimensions per sub-quantizer: a 16-byte
granule of a decoded row is one centroid), so its operands are bit for bit the image's — and the results are the table scan's,
the image mode's and the oracle's, bit for bit.  Every case needs the new entry point."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks

pytestmark = pytest.mark.gpu

SCOPE = "pq_codes_gemm"   # the profile scope of the code-gathered GEMM


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


@pytest.fixture
def nominate_always():
    """the library nominates from its pair threshold up; the tests' segments are smaller"""
    hooks.set_hook("VG_PQ_NOM_ALWAYS", 1)
    yield
    hooks.set_hook("VG_PQ_NOM_ALWAYS", 0)


def _random_pq(rng, dim, m, k=256):
    sd = dim // m
    opq = o.ProductQuantizer(dim, m, k)
    cb = rng.integers(-128, 128, m * k * sd).astype(np.int8)
    scales = (rng.random(m) * 0.02 + 0.005).astype(np.float32)
    offsets = ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32)
    opq.set_codebooks(cb, scales, offsets)
    return opq


def _mk(vg, ctx, opq, codes, n):
    pq = vg.ProductQuantizer(ctx, opq.dim, opq.m, opq.k)
    pq.set_codebooks(opq.codebooks, opq.scales, opq.offsets)
    idx = vg.Index(ctx, n, opq.dim, vg.Metric.L2)
    idx.set_pq_codes(pq, codes)
    return pq, idx


def _decoded(opq, codes):
    """ProductQuantizer.Decode of every row (pq.go:185-229): float32(int8) * scale, + offset, two rounded operations"""
    sd = opq.dim // opq.m
    cb = np.asarray(opq.codebooks, np.int8).reshape(opq.m, opq.k, sd).astype(np.float32)
    v = cb * np.asarray(opq.scales, np.float32)[:, None, None]
    v = (v + np.asarray(opq.offsets, np.float32)[:, None, None]).astype(np.float32)
    return v[np.arange(opq.m)[None, :], codes].reshape(codes.shape[0], opq.dim)


def _clustered_codes(rng, n, m, clusters=40, flip=0.3):
    """codes around a few prototypes: neighbours exist (a uniform draw has none in 96 sub-spaces)"""
    proto = rng.integers(0, 256, (clusters, m)).astype(np.uint8)
    codes = proto[rng.integers(0, clusters, n)]
    noise = rng.integers(0, 256, (n, m)).astype(np.uint8)
    return np.where(rng.random((n, m)) < flip, noise, codes).astype(np.uint8)


def _queries(rng, x, nq):
    q = (x[rng.integers(0, x.shape[0], nq)] + rng.standard_normal((nq, x.shape[1])).astype(np.float32) * 0.05).astype(np.float32)
    q[1] = x[100]   # exactly a decoded row (one of the ten tied ones)
    return q


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def _launches(ctx, search):
    """search()'s result and how often the code-gathered GEMM ran in it"""
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SCOPE)
        r = search()
        return r, ctx.profile_read(SCOPE)[0]
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("n,m,nq,k", [(9000, 96, 300, 10),    # 12 K steps, two query tiles, last row tile partial
                                      (4097, 8, 130, 10),     # one K step; the first size with a sample
                                      (4096, 16, 130, 48),    # no sample, everything appended; the pick's last k
                                      (700, 24, 140, 49),     # three steps = one lap of the ring; everything re-scored
                                      (5000, 12, 200, 100),   # m % 8 != 0: zero granules, unaligned code reads
                                      (300, 1, 129, 5),       # one sub-quantizer; just above one row tile
                                      (12000, 32, 257, 256)])  # k at the limit; a third query tile holding one query
def test_parity_with_scan_image_and_oracle(vg, ctx, nominate_always, n, m, nq, k):
    dim = 8 * m
    rng = np.random.default_rng(n + dim + m)
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    codes[100:110] = codes[100]                   # ties
    codes[200], codes[201], codes[n - 1] = 0, 255, 255   # the codebook's first and last entries in every sub-quantizer
    codes[202, ::2], codes[202, 1::2] = 0, 255
    pq, idx = _mk(vg, ctx, opq, codes, n)
    q = _queries(rng, _decoded(opq, codes), nq)
    plain = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination(True)
    image = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination_from_codes(True)
    got, launches = _launches(ctx, lambda: idx.search_pq_adc(q, k))
    assert launches >= 1, "the batch kept the table scan"
    assert _same(plain, got) and _same(image, got)
    for i in (0, 1, nq // 2, nq - 1):
        eid, esc = o.flat_search_pq(opq, codes, q[i], k)
        assert np.array_equal(got[0][i, :eid.size], eid) and np.array_equal(bits(got[1][i, :eid.size]), bits(esc))


def test_batches_the_mode_does_not_take(vg, ctx, nominate_always):
    rng = np.random.default_rng(5)
    n, m = 6000, 16
    opq = _random_pq(rng, 8 * m, m)
    codes = _clustered_codes(rng, n, m)
    pq, idx = _mk(vg, ctx, opq, codes, n)
    q = _queries(rng, _decoded(opq, codes), 128)
    plain = idx.search_pq_adc(q, 10)
    idx.enable_pq_nomination_from_codes(True)
    for nq in (128, 7):
        got, launches = _launches(ctx, lambda: idx.search_pq_adc(q[:nq], 10))
        assert launches == 0
        assert _same((plain[0][:nq], plain[1][:nq]), got)


def test_far_queries_and_non_finite_values(vg, ctx, nominate_always):
    """test_nomination_with_far_queries_and_non_finite_values's inputs (tests/test_gpu_adc.py) in a batch this mode takes: a far
    query, NaN / Inf queries, an all-zero query, then a NaN scale (norm_max = +Inf: every proof fails) — on = off, bit for bit"""
    rng = np.random.default_rng(321)
    n, dim, m, nq, k = 12000, 128, 16, 140, 10
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    x = _decoded(opq, codes)
    q = (x[rng.integers(0, n, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.05).astype(np.float32)
    q[2] = rng.standard_normal(dim).astype(np.float32) * 1000.0
    q[3, 5] = np.nan
    q[4, :] = np.inf
    q[5, 7] = -np.inf
    q[6] = 0.0
    for poison in (False, True):
        if poison:
            sc = np.array(opq.scales, np.float32)
            sc[3] = np.nan
            opq.set_codebooks(opq.codebooks, sc, opq.offsets)
        pq, idx = _mk(vg, ctx, opq, codes, n)
        plain = idx.search_pq_adc(q, k)
        idx.enable_pq_nomination_from_codes(True)
        got, launches = _launches(ctx, lambda: idx.search_pq_adc(q, k))
        assert launches >= 1
        assert _same(plain, got), poison
        if not poison:
            for i in (0, 2, 6, nq - 1):
                eid, esc = o.flat_search_pq(opq, codes, q[i], k)
                assert np.array_equal(got[0][i], eid) and np.array_equal(bits(got[1][i]), bits(esc))


def _cap(n, dim):
    dim_pad = (dim + 63) // 64 * 64
    return n * (4 + dim_pad // 32) + (dim_pad // 8 + 1) * 256 * 16 + 4096


def test_memory_and_lifetime(vg, ctx, nominate_always):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(77)
    n, dim, m, nq, k = 9000, 128, 16, 160, 10
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    pq, idx = _mk(vg, ctx, opq, codes, n)
    q = _queries(rng, _decoded(opq, codes), nq)
    assert idx.pq_nomination_info() == (0, 0)
    plain = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination_from_codes(True)
    mode, held = idx.pq_nomination_info()
    assert mode == 2 and n * 4 <= held <= _cap(n, dim)
    assert held == n * 4 + 4 + (dim // 8) * 256 * 16          # the norms, norm_max, the decoded codebook: no row image
    from_codes = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination(True)                            # 2 -> 1: the modes are exclusive
    mode, held = idx.pq_nomination_info()
    assert mode == 1 and held >= n * dim * 2
    image = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination_from_codes(True)                 # 1 -> 2
    assert idx.pq_nomination_info()[0] == 2
    again, launches = _launches(ctx, lambda: idx.search_pq_adc(q, k))
    assert launches >= 1 and _same(plain, from_codes) and _same(plain, image) and _same(plain, again)
    # device queries and outputs on a caller's own stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q).cuda()
        out = (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"))
        idx.search_pq_adc(dq, k, out=out, stream=s)
    s.synchronize()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), plain[0]) and np.array_equal(bits(out[1].cpu().numpy()), bits(plain[1]))
    idx.enable_pq_nomination_from_codes(False)
    assert idx.pq_nomination_info() == (0, 0)
    assert _launches(ctx, lambda: idx.search_pq_adc(q, k))[1] == 0
    # new codes drop the state
    idx.enable_pq_nomination_from_codes(True)
    codes2 = _clustered_codes(rng, n, m)
    idx.set_pq_codes(pq, codes2)
    assert idx.pq_nomination_info() == (0, 0)
    got = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination_from_codes(True)
    re_enabled, launches = _launches(ctx, lambda: idx.search_pq_adc(q, k))
    assert launches >= 1 and _same(got, re_enabled)
    for i in (0, nq - 1):
        eid, esc = o.flat_search_pq(opq, codes2, q[i], k)
        assert np.array_equal(re_enabled[0][i], eid) and np.array_equal(bits(re_enabled[1][i]), bits(esc))
    # refusals: no codes; K = 64; sub-vectors of 4 dimensions
    with pytest.raises(vg.VecgoHipError):
        vg.Index(ctx, 10, dim, vg.Metric.L2).enable_pq_nomination_from_codes(True)
    o64 = _random_pq(rng, dim, m, k=64)
    p64 = vg.ProductQuantizer(ctx, dim, m, 64)
    p64.set_codebooks(o64.codebooks, o64.scales, o64.offsets)
    i64 = vg.Index(ctx, 100, dim, vg.Metric.L2)
    i64.set_pq_codes(p64, rng.integers(0, 64, (100, m)).astype(np.uint8))
    with pytest.raises(vg.VecgoHipError) as e:
        i64.enable_pq_nomination_from_codes(True)
    assert e.value.status == -5
    o4 = _random_pq(rng, 64, 16)
    p4, i4 = _mk(vg, ctx, o4, rng.integers(0, 256, (100, 16)).astype(np.uint8), 100)
    with pytest.raises(vg.VecgoHipError) as e:
        i4.enable_pq_nomination_from_codes(True)
    assert e.value.status == -5 and "4" in e.value.message
    assert i4.pq_nomination_info() == (0, 0)


def test_each_entry_point_switches_its_own_mode(vg, ctx, nominate_always):
    """enable_X(False) drops mode X alone; a refused enable_X(True) leaves a different active mode as it was"""
    rng = np.random.default_rng(78)
    n, dim, m, nq, k = 9000, 128, 16, 160, 10
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    pq, idx = _mk(vg, ctx, opq, codes, n)
    q = _queries(rng, _decoded(opq, codes), nq)
    plain = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination_from_codes(True)
    idx.enable_pq_nomination(False)                           # not its mode: mode 2 stays, and still takes the batch
    assert idx.pq_nomination_info()[0] == 2
    got, launches = _launches(ctx, lambda: idx.search_pq_adc(q, k))
    assert launches >= 1 and _same(plain, got)
    idx.enable_pq_nomination(True)
    held = idx.pq_nomination_info()
    assert held == (1, n * (dim * 2 + 4) + 4)                 # the image (dim_pad = dim here), the norms, norm_max
    idx.enable_pq_nomination_from_codes(False)                # not its mode: mode 1 stays
    assert idx.pq_nomination_info() == held
    assert _same(plain, idx.search_pq_adc(q, k))
    # sub-vectors of 4 dimensions: the image is on, from the codes is refused and the image stays
    o4 = _random_pq(rng, 64, 16)
    p4, i4 = _mk(vg, ctx, o4, rng.integers(0, 256, (100, 16)).astype(np.uint8), 100)
    i4.enable_pq_nomination(True)
    held = i4.pq_nomination_info()
    assert held == (1, 100 * (64 * 2 + 4) + 4)
    with pytest.raises(vg.VecgoHipError) as e:
        i4.enable_pq_nomination_from_codes(True)
    assert e.value.status == -5
    assert i4.pq_nomination_info() == held


def test_reorder_moves_the_norms_with_the_codes(vg, ctx, nominate_always):
    """vg_vamana_reorder_bfs on an index with the mode on (as the image's case in tests/test_gpu_vamana_reorder.py): afterwards the
    nominated batch equals the table scan over the permuted codes and a fresh index of them"""
    rng = np.random.default_rng(21)
    n, dim, m, r, nq, k = 6000, 128, 16, 24, 160, 10
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    x = _decoded(opq, codes)
    q = _queries(rng, x, nq)
    g = rng.integers(0, n, (n, r)).astype(np.uint32)
    g[rng.random((n, r)) < 0.3] = 0xFFFFFFFF
    pq, idx = _mk(vg, ctx, opq, codes, n)
    idx.set_vectors(x)
    idx.enable_pq_nomination_from_codes(True)
    idx.set_vamana_graph(g, n // 3)
    perm, inv = idx.reorder_vamana_bfs()
    assert idx.pq_nomination_info()[0] == 2 and not np.array_equal(perm, np.arange(n))
    got, launches = _launches(ctx, lambda: idx.search_pq_adc(q, k))
    assert launches >= 1
    _, fresh = _mk(vg, ctx, opq, codes[perm], n)
    assert _same(fresh.search_pq_adc(q, k), got)
    idx.enable_pq_nomination_from_codes(False)
    assert _same(idx.search_pq_adc(q, k), got)


def test_inserts_are_refused(vg, ctx):
    rng = np.random.default_rng(9)
    n, dim, m = 500, 64, 8
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    rows = rng.standard_normal((4, dim)).astype(np.float32)
    for graph in ("hnsw", "vamana"):
        pq = vg.ProductQuantizer(ctx, dim, m, 256)
        pq.set_codebooks(opq.codebooks, opq.scales, opq.offsets)
        idx = vg.Index(ctx, n, dim, vg.Metric.L2)
        idx.set_vectors(_decoded(opq, codes))
        if graph == "hnsw":
            idx.build_hnsw(m=8, ef_construction=32, max_batch=64, growth_div=16)
        else:
            idx.set_vamana_graph(rng.integers(0, n, (n, 8)).astype(np.uint32), 0)
        idx.set_pq_codes(pq, codes)
        idx.enable_pq_nomination_from_codes(True)
        with pytest.raises(vg.VecgoHipError) as e:
            if graph == "hnsw":
                idx.insert_hnsw(rows, m=8, ef_construction=32, max_batch=64, growth_div=16)
            else:
                idx.insert_vamana(rows, r=8, l=16)
        assert e.value.status == -5 and "the index holds" in e.value.message, graph
        assert idx.n == n and idx.pq_nomination_info()[0] == 2
