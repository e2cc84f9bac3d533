"""vg_index_enable_sq8_nomination_from_codes: the SQ8 batch nomination WITHOUT the image of the dequantised rows.  The nomination
GEMM multiplies the queries scaled by the inverse scales, bf16(q_d * inv_d), by the centred codes, bf16(code - 128) — exact —
which its row tiles convert from the index's code tiles in registers (flat_gemm_sq8_big_kernel); the re-score is the scan's, the
proof takes the score space's per-query constant back — and the results are the scan's, the image mode's and the oracle's, bit for
bit.  Every case needs the new entry point."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks

pytestmark = pytest.mark.gpu

SCOPE = "sq8_codes_gemm"   # the profile scope of the GEMM on the code tiles
L2, DOT = 0, 2


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
    hooks.set_hook("VG_SQ8_NOM_CODES_ALWAYS", 1)
    yield
    hooks.set_hook("VG_SQ8_NOM_CODES_ALWAYS", 0)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def _launches(ctx, search):
    """search()'s result and how often the GEMM on the code tiles ran in it"""
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SCOPE)
        r = search()
        return r, ctx.profile_read(SCOPE)[0]
    finally:
        ctx.profile_enable(False)


def _quantizers(vg, ctx, x, bounds=None):
    """the library's quantizer trained on x (or with the given bounds) and the oracle's with the same parameters"""
    dim = x.shape[1]
    sq = vg.ScalarQuantizer(ctx, dim)
    if bounds is None:
        sq.train(x)
    else:
        sq.set_bounds(*bounds)
    ref = o.ScalarQuantizer(dim)
    for dst, src in zip((ref.mins, ref.maxs, ref.scales, ref.inv_scales), sq.params()):
        dst[:] = src
    ref.trained = True
    return sq, ref


def _index(vg, ctx, sq, codes, metric):
    idx = vg.Index(ctx, codes.shape[0], codes.shape[1], vg.Metric(metric))
    idx.set_sq8_codes(sq, codes)
    return idx


def _oracle(ref, x, codes, metric, q, k):
    if metric == L2:
        return o.flat_search_sq8(ref, codes, q, k)
    return o.FlatSegment(x, x.shape[1], metric=metric, sq=ref, codes=codes).search(q, k)


SHAPES = [(9000, 128, 300, 10),     # two query tiles, the last row tile partial
          (4097, 64, 130, 10),      # one K step; the first size with a sample
          (4096, 64, 130, 48),      # no sample; everything appended; the pick's last k
          (700, 192, 140, 49),      # three steps, one lap of the ring; everything re-scored
          (5000, 100, 200, 100),    # dim % 16 and % 64 != 0: a partial group, zero groups
          (300, 16, 129, 5),        # one group; just above one row tile
          (12000, 128, 257, 256),   # k at the limit; a third query tile holding one query
          (70000, 64, 300, 10),     # more tiles than workgroups: a workgroup's stream crosses tile boundaries
          (3000, 768, 140, 10)]     # twelve steps


@pytest.mark.parametrize("metric", [L2, DOT], ids=["L2", "Dot"])
@pytest.mark.parametrize("n,dim,nq,k", SHAPES)
def test_parity_with_scan_image_and_oracle(vg, ctx, nominate_always, n, dim, nq, k, metric):
    rng = np.random.default_rng(n + dim + metric)
    cent = rng.standard_normal((30, dim)).astype(np.float32) * 2
    x = (cent[rng.integers(0, 30, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.5).astype(np.float32)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    codes[100:110] = codes[100]                               # ties
    codes[200], codes[201], codes[n - 1] = 0, 255, codes[7]   # an all-0 and an all-255 row; the last row equal to an early one
    idx = _index(vg, ctx, sq, codes, metric)
    q = (cent[rng.integers(0, 30, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.5).astype(np.float32)
    q[1] = ref.decode(codes[100])                             # exactly a row (one of the ten tied ones)
    q[2] = ref.decode(codes[n - 1])
    plain = idx.search_sq8(q, k)
    idx.enable_sq8_nomination(True)
    image = idx.search_sq8(q, k)
    idx.enable_sq8_nomination_from_codes(True)
    got, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
    assert launches >= 1, "the batch kept the scan"
    assert _same(plain, got) and _same(image, got)
    for i in (0, 1, 2, nq // 2, nq - 1):
        eid, esc = _oracle(ref, x, codes, metric, q[i], k)
        assert np.array_equal(got[0][i, :eid.size], eid) and np.array_equal(bits(got[1][i, :eid.size]), bits(esc))


@pytest.mark.parametrize("metric", [L2, DOT], ids=["L2", "Dot"])
def test_planted_granules(vg, ctx, nominate_always, metric):
    """query (slot, g) is row `slot` of a 256-row tile, dequantised; a decoy row elsewhere equals it except in the 16-dimension
    group g.  Every lane's granule of every K step decides one of these pairs: the nominated result ranks all of them as the scan
    does, and hardly any query needed the scan."""
    rng = np.random.default_rng(4 + metric)
    n, dim, k = 8192, 128, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    q = np.empty((2048, dim), np.float32)
    for slot in range(256):
        for g in range(8):
            t = g * 2 + (slot & 1)                      # targets in tiles 0 .. 15, decoys in 16 .. 31, the same slot
            row, decoy = t * 256 + slot, (16 + t) * 256 + slot
            codes[decoy] = codes[row]
            codes[decoy, g * 16:(g + 1) * 16] ^= np.uint8(1 << (slot % 3))     # the group's 16 codes moved by 1, 2 or 4
            q[slot * 8 + g] = ref.decode(codes[row])
    idx = _index(vg, ctx, sq, codes, metric)
    plain = idx.search_sq8(q, k)
    idx.enable_sq8_nomination_from_codes(True)
    got, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
    assert launches >= 1
    bad = np.flatnonzero((plain[0] != got[0]).any(1) | (bits(plain[1]) != bits(got[1])).any(1))
    assert bad.size == 0, [(int(b) // 8, int(b) % 8) for b in bad[:10]]      # (slot, group)
    if metric == L2:                                    # the row itself first, then its decoy
        slots, groups = np.divmod(np.arange(2048), 8)
        t = groups * 2 + (slots & 1)
        assert np.array_equal(got[0][:, 0], (t * 256 + slots).astype(np.uint32))
        assert np.array_equal(got[0][:, 1], ((16 + t) * 256 + slots).astype(np.uint32))
    rescanned = idx.sq8_nomination_info()[2]
    print(f"planted granules metric={metric}: rescanned {rescanned} of 2048")
    assert rescanned <= 2048 // 20


@pytest.mark.parametrize("metric", [L2, DOT], ids=["L2", "Dot"])
@pytest.mark.parametrize("n,dim,nq,k", [SHAPES[0], SHAPES[3], SHAPES[7], SHAPES[8]])
def test_the_nomination_is_doing_the_work(vg, ctx, nominate_always, n, dim, nq, k, metric):
    """i.i.d. normal rows, queries = a row + 0.05 normal: at most 5 % of the queries fall back to the scan (a numpy emulation of
    sample threshold, k-th score and margin on these inputs gave none); a nomination whose every proof failed would pass the parity
    tests too"""
    rng = np.random.default_rng(n + metric)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    idx = _index(vg, ctx, sq, codes, metric)
    q = (x[rng.integers(0, n, nq)] + 0.05 * rng.standard_normal((nq, dim)).astype(np.float32)).astype(np.float32)
    plain = idx.search_sq8(q, k)
    idx.enable_sq8_nomination_from_codes(True)
    assert idx.sq8_nomination_info()[2] == 0
    got, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
    rescanned = idx.sq8_nomination_info()[2]
    print(f"n={n} dim={dim} nq={nq} k={k} metric={metric}: rescanned {rescanned} of {nq}")
    assert launches >= 1 and _same(plain, got)
    assert rescanned <= nq // 20
    idx.enable_sq8_nomination_from_codes(True)          # enabling again starts the count again
    assert idx.sq8_nomination_info()[2] == 0


@pytest.mark.parametrize("metric", [L2, DOT], ids=["L2", "Dot"])
def test_batches_the_mode_does_not_take(vg, ctx, nominate_always, metric):
    """128 queries, 7 queries, a filtered batch and a probed search keep the scan: no launch of the new GEMM, the scan's results"""
    from tests.test_gpu_probe import partitioned
    rng = np.random.default_rng(5 + metric)
    n, dim, parts, nq, k = 12000, 64, 6, 200, 10
    x, cent, off = partitioned(rng, n, dim, parts, metric)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    idx = _index(vg, ctx, sq, codes, metric)
    pidx = _index(vg, ctx, sq, codes, metric)
    pidx.set_partitions(cent, off)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    masks = rng.random((nq, n)) < 0.4

    def run():
        return [idx.search_sq8(q[:128], k), idx.search_sq8(q[:7], k), idx.search_flat_filtered(q, k, masks, 0, scan=idx.SCAN_SQ8),
                idx.search_flat_filtered(q, k, masks[0], 0, scan=idx.SCAN_SQ8), pidx.search_flat_probed(q, k, 2, scan=pidx.SCAN_SQ8),
                pidx.search_flat_probed(q, k, parts, scan=pidx.SCAN_SQ8)]

    plain, whole = run(), idx.search_sq8(q, k)
    idx.enable_sq8_nomination_from_codes(True)
    pidx.enable_sq8_nomination_from_codes(True)
    got, launches = _launches(ctx, run)
    assert launches == 0
    assert all(_same(a, b) for a, b in zip(plain, got))
    assert idx.sq8_nomination_info()[2] == 0 and pidx.sq8_nomination_info()[2] == 0
    taken, launches = _launches(ctx, lambda: idx.search_sq8(q, k))      # and the batch it does take, on the same index
    assert launches >= 1 and _same(whole, taken)


@pytest.mark.parametrize("metric", [L2, DOT], ids=["L2", "Dot"])
def test_far_queries_and_non_finite_values(vg, ctx, nominate_always, metric):
    """a far query, NaN / Inf queries, an all-zero query, then a NaN min (norm_max = +Inf: every proof fails and every query is
    counted as rescanned) — on = off, bit for bit"""
    rng = np.random.default_rng(321 + metric)
    n, dim, nq, k = 12000, 128, 140, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = (x[rng.integers(0, n, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.05).astype(np.float32)
    q[2] = rng.standard_normal(dim).astype(np.float32) * 1000.0
    q[3, 5] = np.nan
    q[4, :] = np.inf
    q[5, 7] = -np.inf
    q[6] = 0.0
    for poison in (False, True):
        if poison:
            mins, maxs = x.min(0).copy(), x.max(0).copy() + 1e-3
            mins[3] = np.nan
            sq, ref = _quantizers(vg, ctx, x, (mins, maxs))
            codes = rng.integers(0, 256, (n, dim)).astype(np.uint8)
        else:
            sq, ref = _quantizers(vg, ctx, x)
            codes = sq.encode(x)
        idx = _index(vg, ctx, sq, codes, metric)
        plain = idx.search_sq8(q, k)
        idx.enable_sq8_nomination_from_codes(True)
        got, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
        assert launches >= 1
        assert np.array_equal(plain[0], got[0]), poison
        assert np.all((bits(plain[1]) == bits(got[1])) | (np.isnan(plain[1]) & np.isnan(got[1]))), poison
        rescanned = idx.sq8_nomination_info()[2]
        if poison:
            assert rescanned == nq
        else:
            assert 3 <= rescanned <= 3 + nq // 20       # the NaN and the two Inf queries, and hardly any other
            for i in (0, 2, 6, nq - 1):
                eid, esc = _oracle(ref, x, codes, metric, q[i], k)
                assert np.array_equal(got[0][i], eid) and np.array_equal(bits(got[1][i]), bits(esc))


def test_memory_and_lifetime(vg, ctx, nominate_always):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(77)
    n, dim, nq, k = 9000, 100, 160, 10
    dim_pad = (dim + 63) // 64 * 64
    x = rng.standard_normal((n, dim)).astype(np.float32)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    idx = _index(vg, ctx, sq, codes, L2)
    q = (x[rng.integers(0, n, nq)] + 0.05 * rng.standard_normal((nq, dim)).astype(np.float32)).astype(np.float32)
    assert idx.sq8_nomination_info() == (0, 0, 0)
    plain = idx.search_sq8(q, k)
    idx.enable_sq8_nomination_from_codes(True)
    mode, held, _ = idx.sq8_nomination_info()
    assert mode == 2 and n * 4 <= held <= n * 4 + 64 * dim_pad + 4096       # no term in rows x dim
    assert held == n * 4 + 4 + (dim_pad + 1) * 4                            # the norms, norm_max, mid and H2
    from_codes = idx.search_sq8(q, k)
    idx.enable_sq8_nomination(True)                           # 2 -> 1: the modes are exclusive
    mode, held, _ = idx.sq8_nomination_info()
    assert (mode, held) == (1, n * (dim_pad * 2 + 4) + 4)
    image, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
    assert launches == 0
    idx.enable_sq8_nomination_from_codes(False)               # not its mode: mode 1 stays
    assert idx.sq8_nomination_info()[:2] == (1, held)
    idx.enable_sq8_nomination_from_codes(True)                # 1 -> 2
    assert idx.sq8_nomination_info()[0] == 2
    idx.enable_sq8_nomination(False)                          # not its mode: mode 2 stays, and still takes the batch
    assert idx.sq8_nomination_info()[0] == 2
    again, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
    assert launches >= 1 and _same(plain, from_codes) and _same(plain, image) and _same(plain, again)
    # device queries and outputs on a caller's own stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dq = torch.from_numpy(q).cuda()
        out = (torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"))
        idx.search_sq8(dq, k, out=out, stream=s)
    s.synchronize()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), plain[0]) and np.array_equal(bits(out[1].cpu().numpy()), bits(plain[1]))
    idx.enable_sq8_nomination_from_codes(False)
    assert idx.sq8_nomination_info() == (0, 0, 0)
    assert _launches(ctx, lambda: idx.search_sq8(q, k))[1] == 0
    # new codes drop the state
    idx.enable_sq8_nomination_from_codes(True)
    codes2 = sq.encode(rng.standard_normal((n, dim)).astype(np.float32))
    idx.set_sq8_codes(sq, codes2)
    assert idx.sq8_nomination_info() == (0, 0, 0)
    got = idx.search_sq8(q, k)
    idx.enable_sq8_nomination_from_codes(True)
    re_enabled, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
    assert launches >= 1 and _same(got, re_enabled)
    for i in (0, nq - 1):
        eid, esc = o.flat_search_sq8(ref, codes2, q[i], k)
        assert np.array_equal(re_enabled[0][i], eid) and np.array_equal(bits(re_enabled[1][i]), bits(esc))
    # refusal: no codes
    with pytest.raises(vg.VecgoHipError):
        vg.Index(ctx, 10, dim, vg.Metric.L2).enable_sq8_nomination_from_codes(True)


def test_reorder_moves_the_norms_with_the_codes(vg, ctx, nominate_always):
    """vg_vamana_reorder_bfs on an index with the mode on: mode 2 stays, and the nominated batch equals a fresh index of the
    permuted codes"""
    rng = np.random.default_rng(21)
    n, dim, r, nq, k = 6000, 128, 24, 160, 10
    x = rng.standard_normal((n, dim)).astype(np.float32) * (1.0 + rng.random((n, 1)).astype(np.float32))   # norms that differ
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    q = (x[rng.integers(0, n, nq)] + 0.05 * rng.standard_normal((nq, dim)).astype(np.float32)).astype(np.float32)
    g = rng.integers(0, n, (n, r)).astype(np.uint32)
    g[rng.random((n, r)) < 0.3] = 0xFFFFFFFF
    idx = _index(vg, ctx, sq, codes, L2)
    idx.set_vectors(x)
    idx.enable_sq8_nomination_from_codes(True)
    idx.set_vamana_graph(g, n // 3)
    perm, inv = idx.reorder_vamana_bfs()
    assert idx.sq8_nomination_info()[0] == 2 and not np.array_equal(perm, np.arange(n))
    got, launches = _launches(ctx, lambda: idx.search_sq8(q, k))
    assert launches >= 1 and idx.sq8_nomination_info()[2] <= nq // 20
    fresh = _index(vg, ctx, sq, codes[perm], L2)
    assert _same(fresh.search_sq8(q, k), got)
    idx.enable_sq8_nomination_from_codes(False)
    assert _same(idx.search_sq8(q, k), got)


def test_inserts_and_flat_build_are_refused(vg, ctx):
    rng = np.random.default_rng(9)
    n, dim = 500, 64
    x = rng.standard_normal((n, dim)).astype(np.float32)
    rows = rng.standard_normal((4, dim)).astype(np.float32)
    for what in ("hnsw", "vamana", "flat_build"):
        sq, ref = _quantizers(vg, ctx, x)
        idx = vg.Index(ctx, n, dim, vg.Metric.L2)
        idx.set_vectors(x)
        if what == "hnsw":
            idx.build_hnsw(m=8, ef_construction=32, max_batch=64, growth_div=16)
        elif what == "vamana":
            idx.set_vamana_graph(rng.integers(0, n, (n, 8)).astype(np.uint32), 0)
        idx.set_sq8_codes(sq, sq.encode(x))
        idx.enable_sq8_nomination_from_codes(True)
        with pytest.raises(vg.VecgoHipError) as e:
            if what == "hnsw":
                idx.insert_hnsw(rows, m=8, ef_construction=32, max_batch=64, growth_div=16)
            elif what == "vamana":
                idx.insert_vamana(rows, r=8, l=16)
            else:
                idx.flat_build(4)
        assert e.value.status == -5 and "the index holds" in e.value.message, what
        assert idx.n == n and idx.sq8_nomination_info()[0] == 2
