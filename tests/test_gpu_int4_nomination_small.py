"""vg_index_enable_int4_nomination with on = 2: vg_search_int4 batches of 5 .. 128 queries through the matrix-core nomination on the
tile of one query tile (flat_gemm_int4_small_kernel: the codes read from global memory into the matrix instruction's registers) —
against the search with the mode off and tests/int4_search_ref.py, ids and score bits.  Every case asserts which GEMM scope ran."""
import numpy as np
import pytest

from tests import int4_search_ref as ref
from tests.test_gpu_int4_search import ctx, vg  # noqa: F401  (the module's fixtures)
from tests.test_gpu_int4_nomination import _index, _near, nominate_always  # noqa: F401  (its helpers; VG_INT4_NOM_ALWAYS on)

pytestmark = pytest.mark.gpu
SMALL, BIG = "int4_codes_gemm_small", "int4_codes_gemm"   # the profile scopes of the two GEMMs on the nibble codes


def _on_equals_off(ctx, idx, iq, codes, runs, small=True, launched=SMALL):
    """the codes set, every run with the mode off, then on (mode 2, or 1): the same ids and score bits (NaN == NaN); of the two GEMM
    scopes only `launched` (or none) ran"""
    idx.set_int4_codes(iq, codes)
    off = [r() for r in runs]
    idx.enable_int4_nomination(True, small_batches=small)
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SMALL), ctx.profile_read(BIG)
        on = [r() for r in runs]
        ran = {s for s in (SMALL, BIG) if ctx.profile_read(s)[0] >= 1}
    finally:
        ctx.profile_enable(False)
    assert ran == ({launched} if launched else set()), ran
    for a, b in zip(off, on):
        for qi in range(a[0].shape[0]):
            ref.assert_row(b[0][qi], b[1][qi], a[0][qi], a[1][qi], ("query", qi))
    return on[0]


CASES = [(4097, 64, 10, 5),        # the first size with a sample; one block holding five queries
         (4096, 64, 48, 32),       # no sample, everything appended
         (300, 32, 5, 33),         # less than one tile, one 16-byte unit a row
         (5000, 96, 100, 64),      # dim % 64 == 32: lane half 1's last unit is zeros and is not read
         (700, 192, 49, 65),
         (9000, 128, 10, 96),      # a partial last tile
         (9000, 128, 10, 97),
         (70000, 64, 10, 128),     # more tiles than workgroups
         (3000, 768, 10, 128),     # three whole supersteps; two launches of two blocks
         (3000, 768, 10, 96),      # ... and three blocks in one
         (12000, 128, 256, 33),    # k at the limit
         (5000, 96, 100, 128)]


@pytest.mark.parametrize("n,dim,k,nq", CASES)
def test_parity_with_scan_and_reference(vg, ctx, n, dim, k, nq):
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
    granule g, where one byte's nibbles are swapped (half of the slots) or every nibble is moved by one.  The slots are the 256 (wave,
    row block, lane) of a tile, the granules the halves of every 16-byte load of both lane halves — dim 352: a whole superstep and
    a partial one of three units, which the lane halves split 2 + 1: a wrong nibble order, unit, k-slice or lane-half mapping
    ranks a decoy with its target.  Calls of 128 queries."""
    dim, k = 352, 10
    gn = dim // 16
    n = 2 * gn * 256
    idx, iq, oq, codes = _index(vg, ctx, np.random.default_rng(4).standard_normal((n, dim)).astype(np.float32))
    slots, gs = np.divmod(np.arange(256 * gn), gn)         # targets in tiles 0 .. gn - 1, decoys in gn .. 2 gn - 1, the same slot
    rows, decoys, byte = gs * 256 + slots, (gn + gs) * 256 + slots, gs * 8 + slots % 8
    codes[rows, byte] = (codes[rows, byte] & 0xF0) | ((codes[rows, byte] >> 4) ^ 1)    # that byte's nibbles differ
    codes[decoys] = codes[rows]
    swap = (slots & 2) == 0
    codes[decoys[swap], byte[swap]] = (codes[rows[swap], byte[swap]] << 4) | (codes[rows[swap], byte[swap]] >> 4)
    for j in range(8):
        v = codes[rows[~swap], gs[~swap] * 8 + j].astype(np.int32)
        hi, lo = v >> 4, v & 15
        codes[decoys[~swap], gs[~swap] * 8 + j] = ((np.where(hi < 15, hi + 1, hi - 1) << 4) | np.where(lo < 15, lo + 1, lo - 1)).astype(np.uint8)
    q = np.stack([oq.decode(c) for c in codes[rows]])
    calls = [(lambda a=a: idx.search_int4(q[a:a + 128], k)) for a in range(0, len(rows), 128)]
    idx.set_int4_codes(iq, codes)
    idx.enable_int4_nomination(True, small_batches=True)
    got = np.concatenate([c()[0] for c in calls])
    assert np.array_equal(got[:, 0], rows.astype(np.uint32)) and np.array_equal(got[:, 1], decoys.astype(np.uint32))


@pytest.mark.parametrize("n,dim,k", [(9000, 128, 10), (5000, 96, 100)])
def test_the_nomination_is_doing_the_work(vg, ctx, n, dim, k):
    """i.i.d. normal rows, 128 queries = a row + 0.05 normal: at most 5 % of them fall back to the scan.  The thresholds (the
    nominate_sel_k(k)-th best of every 64th 128-row tile) and Int4Row::eps are the big tile's; a numpy emulation of both and of the
    k-th exact score on these seeds and 128 queries left every proof standing, by a gap of at least 10.7 (eps at most 1.6) at
    9000 x 128, k = 10, and 10.3 (eps at most 1.3) at 5000 x 96, k = 100.  A nomination whose every proof failed would pass the
    parity tests too."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    idx, iq, oq, codes = _index(vg, ctx, x)
    q = _near(rng, x, 128)
    _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q, k)])
    assert idx.int4_nomination_info()[2] <= 128 // 20, idx.int4_nomination_info()


def test_which_batches_the_mode_takes(vg, ctx):
    """mode 1 leaves 7 and 128 queries to the scan; mode 2 leaves it 4 queries, masks and dim 100, gives 129 queries to the big
    tile and reports itself"""
    rng = np.random.default_rng(5)
    n, nq, k = 6000, 129, 10
    for dim in (64, 100):
        idx, iq, oq, codes = _index(vg, ctx, rng.standard_normal((n, dim)).astype(np.float32))
        q, masks = rng.standard_normal((nq, dim)).astype(np.float32), rng.random((nq, n)) < 0.4
        if dim == 100:
            _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q[:100], k)], launched=None)
            continue
        _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q[:7], k), lambda: idx.search_int4(q[:128], k)], small=False, launched=None)
        assert idx.int4_nomination_info()[0] == 1
        _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q[:4], k), lambda: idx.search_int4(q[:100], k, mask=masks[0]),
                                             lambda: idx.search_int4(q[:100], k, mask=masks[:100])], launched=None)
        assert idx.int4_nomination_info()[0] == 2 and idx.int4_nomination_info()[2] == 0
        _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q, k)], launched=BIG)
        _on_equals_off(ctx, idx, iq, codes, [lambda: idx.search_int4(q[:128], k)])


@pytest.mark.parametrize("poison", [False, True])
def test_far_queries_and_non_finite_values(vg, ctx, poison):
    """a far query, NaN / Inf queries, an all-zero query; then the same under a NaN min (norm_max = +Inf: every proof fails and
    every query is counted as rescanned) — on = off, with NaN == NaN"""
    rng = np.random.default_rng(321)
    n, dim, nq, k = 12000, 128, 100, 10
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
