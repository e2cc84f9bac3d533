"""vg_index_enable_int4_nomination: vg_search_int4 batches through the bf16 matrix-core nomination whose row tiles are converted
from the row-major nibble codes (flat_gemm_int4_big_kernel) — against the search with the mode off and tests/int4_search_ref.py, ids
and score bits.  Every case asserts that the GEMM on the codes ran (or did not), and needs the new entry point."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests import int4_search_ref as ref
from tests.test_gpu_int4_search import ctx, vg  # noqa: F401  (the module's fixtures)

pytestmark = pytest.mark.gpu
SCOPE = "int4_codes_gemm"   # the profile scope of the GEMM on the nibble codes


@pytest.fixture(autouse=True)
def nominate_always():
    """the library nominates from its pair threshold up; the tests' segments are smaller"""
    hooks.set_hook("VG_INT4_NOM_ALWAYS", 1)
    yield
    hooks.set_hook("VG_INT4_NOM_ALWAYS", 0)


def _index(vg, ctx, x):
    """an index for x's codes; the library's quantizer trained on x and the oracle's; the codes"""
    iq, oq = vg.Int4Quantizer(ctx, x.shape[1]), o.Int4Quantizer(x.shape[1])
    iq.train(x)
    oq.train(x)
    return vg.Index(ctx, x.shape[0], x.shape[1]), iq, oq, iq.encode(x)


def _launches(ctx, run):
    """run()'s result and how often the GEMM on the codes ran in it"""
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SCOPE)
        return run(), ctx.profile_read(SCOPE)[0]
    finally:
        ctx.profile_enable(False)


def _on_equals_off(ctx, idx, iq, codes, runs, launched=True):
    """the codes set, every run with the mode off, then on: the same ids and score bits (NaN == NaN), the GEMM launched or not"""
    idx.set_int4_codes(iq, codes)
    off = [r() for r in runs]
    idx.enable_int4_nomination(True)
    on, launches = _launches(ctx, lambda: [r() for r in runs])
    assert (launches >= 1) == launched, launches
    for a, b in zip(off, on):
        for qi in range(a[0].shape[0]):
            ref.assert_row(b[0][qi], b[1][qi], a[0][qi], a[1][qi], ("query", qi))
    return on[0]


def _near(rng, x, nq):
    return (x[rng.integers(0, x.shape[0], nq)] + 0.05 * rng.standard_normal((nq, x.shape[1])).astype(np.float32)).astype(np.float32)


SHAPES = [(9000, 128, 300, 10),     # two query tiles, the last row tile partial
          (4097, 64, 130, 10),      # one K step; the first size with a sample
          (4096, 64, 130, 48),      # no sample; everything appended
          (700, 192, 140, 49),      # three steps
          (5000, 96, 200, 100),     # dim % 64 == 32: the half-step that must be zeros and must not be read
          (300, 32, 129, 5),        # one half-step only
          (12000, 128, 257, 256),   # k at the limit; a third query tile holding one query
          (70000, 64, 300, 10),     # more tiles than workgroups
          (3000, 768, 140, 10)]     # twelve steps


@pytest.mark.parametrize("n,dim,nq,k", SHAPES)
def test_parity_with_scan_and_reference(vg, ctx, n, dim, nq, k):
    rng = np.random.default_rng(n + dim)
    cent = rng.standard_normal((30, dim)).astype(np.float32) * 2
    x = (cent[rng.integers(0, 30, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.5).astype(np.float32)
    idx, iq, oq, codes = _index(vg, ctx, x)
    codes[100:110] = codes[100]                                   # ties
    codes[200], codes[201], codes[n - 1] = 0x00, 0xFF, codes[7]   # an all-0 and an all-15 row; the last row equal to an early one
    q = (cent[rng.integers(0, 30, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.5).astype(np.float32)
    q[1], q[2] = oq.decode(codes[100]), oq.decode(codes[n - 1])   # exactly decoded rows (one of the ten tied ones)
    got = _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q, k)])
    for i in (0, 1, 2, nq // 2, nq - 1):
        ref.assert_row(got[0][i], got[1][i], *ref.expected(ref.row_scores(oq, q[i], codes), k), ("reference", i))


def test_planted_nibbles(vg, ctx):
    """query (slot, g) is row `slot` of a 256-row tile, decoded; a decoy row in another tile equals it except in the 16-element
    granule g, where one byte's nibbles are swapped (half of the slots) or every nibble is moved by one.  Every lane's granules of
    every K step decide one of these pairs: a wrong nibble order, granule slot or half mapping ranks a decoy with its target."""
    n, dim, k = 8192, 128, 10
    idx, iq, oq, codes = _index(vg, ctx, np.random.default_rng(4).standard_normal((n, dim)).astype(np.float32))
    slots, gs = np.divmod(np.arange(2048), 8)
    t = gs * 2 + (slots & 1)                               # targets in tiles 0 .. 15, decoys in 16 .. 31, the same slot
    rows, decoys, byte = t * 256 + slots, (16 + t) * 256 + slots, gs * 8 + slots % 8
    codes[rows, byte] = (codes[rows, byte] & 0xF0) | ((codes[rows, byte] >> 4) ^ 1)    # that byte's nibbles differ
    codes[decoys] = codes[rows]
    swap = (slots & 2) == 0
    codes[decoys[swap], byte[swap]] = (codes[rows[swap], byte[swap]] << 4) | (codes[rows[swap], byte[swap]] >> 4)
    for j in range(8):
        v = codes[rows[~swap], gs[~swap] * 8 + j].astype(np.int32)
        hi, lo = v >> 4, v & 15
        codes[decoys[~swap], gs[~swap] * 8 + j] = ((np.where(hi < 15, hi + 1, hi - 1) << 4) | np.where(lo < 15, lo + 1, lo - 1)).astype(np.uint8)
    q = np.stack([oq.decode(c) for c in codes[rows]])
    got = _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q, k)])
    assert np.array_equal(got[0][:, 0], rows.astype(np.uint32)) and np.array_equal(got[0][:, 1], decoys.astype(np.uint32))


@pytest.mark.parametrize("n,dim,nq,k", [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[8]])
def test_the_nomination_is_doing_the_work(vg, ctx, n, dim, nq, k):
    """i.i.d. normal rows, queries = a row + 0.05 normal: at most 5 % of the queries fall back to the scan.  A numpy emulation of the
    sample threshold (the nominate_sel_k(k)-th best of every 64th 128-row tile), the k-th exact score and Int4Row::eps on these
    inputs left every query's proof standing, by a gap of at least 8.6 (eps at most 1.6) at 9000 x 128, k = 10, and 10.0 (eps 1.3)
    at 5000 x 96, k = 100; 700 and 3000 rows have no sample.  A nomination whose every proof failed would pass the parity tests too."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    idx, iq, oq, codes = _index(vg, ctx, x)
    q = _near(rng, x, nq)
    _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q, k)])
    assert idx.int4_nomination_info()[2] <= nq // 20, idx.int4_nomination_info()


def test_batches_the_mode_does_not_take(vg, ctx):
    """128 queries, 7 queries, a batch mask, per-query masks and dim 100 keep the scan: no launch of the new GEMM, the scan's results"""
    rng = np.random.default_rng(5)
    n, nq, k = 6000, 200, 10
    for dim in (64, 100):
        idx, iq, oq, codes = _index(vg, ctx, rng.standard_normal((n, dim)).astype(np.float32))
        q, masks = rng.standard_normal((nq, dim)).astype(np.float32), rng.random((nq, n)) < 0.4
        runs = [lambda: idx.search_int4(q, k)] if dim == 100 else [lambda: idx.search_int4(q[:128], k), lambda: idx.search_int4(q[:7], k),
                                                                  lambda: idx.search_int4(q, k, mask=masks[0]), lambda: idx.search_int4(q, k, mask=masks)]
        _on_equals_off(ctx, idx, iq, codes, runs, launched=False)
        assert idx.int4_nomination_info()[2] == 0
        if dim == 64:                                      # and the batch it does take, on the same index
            _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q, k)])


@pytest.mark.parametrize("poison", [False, True])
def test_far_queries_and_non_finite_values(vg, ctx, poison):
    """a far query, NaN / Inf queries, an all-zero query; then the same under a NaN min (norm_max = +Inf: every proof fails and
    every query is counted as rescanned) — on = off, with NaN == NaN"""
    rng = np.random.default_rng(321)
    n, dim, nq, k = 12000, 128, 140, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = _near(rng, x, nq)
    q[2] = rng.standard_normal(dim).astype(np.float32) * 1000.0
    q[3, 5], q[4, :], q[5, 7], q[6] = np.nan, np.inf, -np.inf, 0.0
    idx, iq, oq, codes = _index(vg, ctx, x)
    if poison:
        iq.set_params(np.where(np.arange(dim) == 3, np.nan, oq.min).astype(np.float32), oq.diff)
    _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q, k)])
    rescanned = idx.int4_nomination_info()[2]
    assert rescanned == nq if poison else 3 <= rescanned <= 3 + nq // 20, rescanned   # the NaN and the two Inf queries, hardly any other


def test_lifetime_and_reorder(vg, ctx):
    rng = np.random.default_rng(21)
    n, dim, r, nq, k = 6000, 96, 24, 160, 10
    x = rng.standard_normal((n, dim)).astype(np.float32) * (1.0 + rng.random((n, 1)).astype(np.float32))   # norms that differ
    idx, iq, oq, codes = _index(vg, ctx, x)
    with pytest.raises(vg.VecgoHipError):                             # refusal: no codes
        idx.enable_int4_nomination(True)
    idx.set_int4_codes(iq, codes)
    assert idx.int4_nomination_info() == (0, 0, 0)
    idx.enable_int4_nomination(True)
    mode, held, _ = idx.int4_nomination_info()
    assert mode == 1 and n * 4 <= held <= n * 4 + 64 * 128 + 4096     # (dim_pad 128) no term in rows x dim
    idx.search_int4(np.full((nq, dim), np.nan, np.float32), k)
    assert idx.int4_nomination_info()[2] == nq
    idx.enable_int4_nomination(True)                                  # enabling again starts the count again
    assert idx.int4_nomination_info() == (1, held, 0)
    idx.set_int4_codes(iq, codes)                                     # new codes drop the state
    assert idx.int4_nomination_info() == (0, 0, 0)
    g = rng.integers(0, n, (n, r)).astype(np.uint32)                  # vg_vamana_reorder_bfs with the mode on: the norms move with the codes
    g[rng.random((n, r)) < 0.3] = 0xFFFFFFFF
    idx.enable_int4_nomination(True)
    idx.set_vamana_graph(g, n // 3)
    perm, inv = idx.reorder_vamana_bfs()
    assert idx.int4_nomination_info()[0] == 1 and not np.array_equal(perm, np.arange(n))
    q = _near(rng, x, nq)
    got, launches = _launches(ctx, lambda: idx.search_int4(q, k))
    fresh = vg.Index(ctx, n, dim)
    fresh.set_int4_codes(iq, codes[perm])
    want = fresh.search_int4(q, k)                                    # (the scan)
    assert launches >= 1 and idx.int4_nomination_info()[2] <= nq // 20
    ref.assert_row(got[0], got[1], want[0].reshape(-1), want[1].reshape(-1), "reordered")
