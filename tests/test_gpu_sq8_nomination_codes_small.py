"""vg_index_enable_sq8_nomination_from_codes with on = 2 (mode 3): vg_search_sq8 batches of 5 .. 128 queries through the matrix-core
nomination on the tile of one query tile (flat_gemm_sq8_small_kernel: the code tiles read from global memory into the matrix
instruction's registers) — against the same search with the mode off, ids and score bits, and the oracle.  Every case asserts which
of the two GEMM scopes ran."""
import numpy as np
import pytest

from tests.test_gpu_sq8_nomination_codes import (DOT, L2, _index, _oracle, _quantizers, _same, bits, ctx,  # noqa: F401  (its fixtures
                                                 nominate_always, vg)                                     # and helpers)

pytestmark = pytest.mark.gpu
SMALL, BIG = "sq8_codes_gemm_small", "sq8_codes_gemm"   # the profile scopes of the two GEMMs on the code tiles
METRICS = pytest.mark.parametrize("metric", [L2, DOT], ids=["L2", "Dot"])


def _on_equals_off(ctx, idx, runs, small=True, launched=SMALL, enable=None):
    """every run with the mode off, then on (mode 3, or 2): the same ids and score bits (NaN == NaN); of the two GEMM scopes only
    `launched` (or none) ran"""
    idx.enable_sq8_nomination_from_codes(False)
    off = [r() for r in runs]
    (enable or (lambda: idx.enable_sq8_nomination_from_codes(True, small_batches=small)))()
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SMALL), ctx.profile_read(BIG)
        on = [r() for r in runs]
        ran = {s for s in (SMALL, BIG) if ctx.profile_read(s)[0] >= 1}
    finally:
        ctx.profile_enable(False)
    assert ran == ({launched} if launched else set()), ran
    for a, b in zip(off, on):
        assert np.array_equal(a[0], b[0])
        assert np.all((bits(a[1]) == bits(b[1])) | (np.isnan(a[1]) & np.isnan(b[1])))
    return on


CASES = [(4097, 64, 10, 5),        # the first size with a sample; one block holding five queries
         (4096, 64, 48, 32),       # no sample; everything appended
         (300, 16, 5, 33),         # one group: lane half 1 has no group at all; the second row tile: one real code tile, three past n_tiles
         (5000, 100, 100, 64),     # a partial last group and an odd group count (7)
         (700, 192, 49, 65),       # everything re-scored; three blocks, one holding one query
         (9000, 128, 10, 96),      # three blocks in one launch
         (9000, 128, 10, 97),      # four blocks in one launch
         (3000, 768, 10, 128),     # two launches of two blocks
         (3000, 768, 10, 96),      # three blocks in one launch
         (12000, 128, 256, 33),    # k at the limit
         # more row tiles than workgroups, so that a workgroup's load stream crosses tile boundaries: four blocks at dim 32 take 9 KiB
         # of LDS and 386 registers a lane, one workgroup (four waves, one a SIMD) per compute unit, and the launcher's grid is
         # min(row tiles, 256 compute units x 1); 135461 rows are 530 row tiles of 256 — above 512, should two workgroups fit — the
         # last one of 37 rows: every workgroup walks two or three tiles
         (135461, 32, 10, 128)]


@METRICS
@pytest.mark.parametrize("n,dim,k,nq", CASES)
def test_parity_with_scan_and_oracle(vg, ctx, nominate_always, n, dim, k, nq, metric):
    rng = np.random.default_rng(n + dim + metric)
    cent = rng.standard_normal((30, dim)).astype(np.float32) * 2
    x = (cent[rng.integers(0, 30, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.5).astype(np.float32)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    codes[100:110] = codes[100]                               # ties
    codes[200], codes[201], codes[n - 1] = 0, 255, codes[7]   # an all-0 and an all-255 row; the last row equal to an early one
    idx = _index(vg, ctx, sq, codes, metric)
    q = (cent[rng.integers(0, 30, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.5).astype(np.float32)
    q[1], q[2] = ref.decode(codes[100]), ref.decode(codes[n - 1])   # exactly decoded rows (one of the ten tied ones)
    got = _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q, k)])[0]
    for i in (0, 1, 2, nq // 2, nq - 1):
        eid, esc = _oracle(ref, x, codes, metric, q[i], k)
        assert np.array_equal(got[0][i, :eid.size], eid) and np.array_equal(bits(got[1][i, :eid.size]), bits(esc))


@METRICS
def test_planted_granules(vg, ctx, nominate_always, metric):
    """query (slot, f) is row `slot` of a 256-row tile, dequantised; a decoy row in another tile equals it except in the 8-byte half
    f of a 16-dimension group, where every code is moved by 1, 2 or 4.  The slots are the 256 (wave, row block, lane) of a tile, the
    halves every operand of both lane halves — dim 176: 11 groups, an odd count, six steps.  A wrong byte order, group, half or
    lane-half mapping ranks a decoy with its target.  Calls of 128 queries."""
    dim, k = 176, 10
    hn = dim // 8
    n = 2 * hn * 256
    x = np.random.default_rng(4 + metric).standard_normal((n, dim)).astype(np.float32)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    slots, fs = np.divmod(np.arange(256 * hn), hn)          # targets in tiles 0 .. hn - 1, decoys in hn .. 2 hn - 1, the same slot
    rows, decoys = fs * 256 + slots, (hn + fs) * 256 + slots
    codes[decoys] = codes[rows]
    for j in range(8):
        codes[decoys, fs * 8 + j] ^= (1 << (slots % 3)).astype(np.uint8)
    q = np.stack([ref.decode(c) for c in codes[rows]])
    idx = _index(vg, ctx, sq, codes, metric)
    got = _on_equals_off(ctx, idx, [(lambda a=a: idx.search_sq8(q[a:a + 128], k)) for a in range(0, len(rows), 128)])
    if metric == L2:                                        # the row itself first, then its decoy
        ids = np.concatenate([g[0] for g in got])
        assert np.array_equal(ids[:, 0], rows.astype(np.uint32)) and np.array_equal(ids[:, 1], decoys.astype(np.uint32))


@METRICS
@pytest.mark.parametrize("n,dim,nq0", [(9000, 128, 300), (3000, 768, 140)])
def test_the_nomination_is_doing_the_work(vg, ctx, nominate_always, n, dim, nq0, metric):
    """the arrays of test_gpu_sq8_nomination_codes.py's test of this name at these shapes (the same seed and draws), k = 10, the first
    128 queries: at most 5 % of them fall back to the scan.  A query's sample threshold, k-th score and margin do not depend on the
    batch it is in, so the numpy emulation that test's docstring records (no proof failed for any of its queries) covers these 128,
    which are its first 128; it was NOT run again for this file.  A nomination whose every proof failed would pass the parity tests
    too."""
    rng = np.random.default_rng(n + metric)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    idx = _index(vg, ctx, sq, codes, metric)
    q = (x[rng.integers(0, n, nq0)] + 0.05 * rng.standard_normal((nq0, dim)).astype(np.float32)).astype(np.float32)[:128]
    _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q, 10)])
    assert idx.sq8_nomination_info()[2] <= 128 // 20, idx.sq8_nomination_info()


@METRICS
def test_which_batches_the_mode_takes(vg, ctx, nominate_always, metric):
    """on = 1 leaves 7 and 128 queries to the scan; on = 2 leaves it 4 queries, masks and probed searches, gives 129 queries to the
    big tile and 128 to the small one, and reports mode 3; the image mode and new codes drop it"""
    from tests.test_gpu_probe import partitioned
    rng = np.random.default_rng(5 + metric)
    n, dim, parts, nq, k = 12000, 64, 6, 129, 10
    x, cent, off = partitioned(rng, n, dim, parts, metric)
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    idx, pidx = _index(vg, ctx, sq, codes, metric), _index(vg, ctx, sq, codes, metric)
    pidx.set_partitions(cent, off)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    masks = rng.random((nq, n)) < 0.4
    _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q[:7], k), lambda: idx.search_sq8(q[:128], k)], small=False, launched=None)
    assert idx.sq8_nomination_info()[0] == 2
    _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q[:4], k), lambda: idx.search_flat_filtered(q[:100], k, masks[0], 0, scan=idx.SCAN_SQ8),
                              lambda: idx.search_flat_filtered(q[:100], k, masks[:100], 0, scan=idx.SCAN_SQ8)], launched=None)
    _on_equals_off(ctx, pidx, [lambda: pidx.search_flat_probed(q[:100], k, 2, scan=pidx.SCAN_SQ8),
                               lambda: pidx.search_flat_probed(q[:100], k, parts, scan=pidx.SCAN_SQ8)], launched=None)
    assert idx.sq8_nomination_info()[0] == 3 and idx.sq8_nomination_info()[2] == 0 and pidx.sq8_nomination_info()[0] == 3
    _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q, k)], launched=BIG)
    _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q[:128], k)])
    held = idx.sq8_nomination_info()[1]
    idx.enable_sq8_nomination_from_codes(True)
    assert idx.sq8_nomination_info()[:2] == (2, held)         # nothing more is resident than mode 2's
    idx.enable_sq8_nomination_from_codes(True, small_batches=True)
    _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q[:128], k)], launched=None, enable=lambda: idx.enable_sq8_nomination(True))
    assert idx.sq8_nomination_info()[0] == 1                  # the modes stay exclusive
    idx.enable_sq8_nomination_from_codes(True, small_batches=True)
    idx.set_sq8_codes(sq, codes)
    assert idx.sq8_nomination_info() == (0, 0, 0)


@METRICS
@pytest.mark.parametrize("poison", [False, True])
def test_far_queries_and_non_finite_values(vg, ctx, nominate_always, poison, metric):
    """test_gpu_sq8_nomination_codes.py's queries of this name cut to 100 — a far query, NaN / Inf queries, an all-zero query —
    without and with a NaN min (norm_max = +Inf: every proof fails and every query is counted as rescanned): on = off, NaN == NaN"""
    rng = np.random.default_rng(321 + metric)
    n, dim, nq, k = 12000, 128, 100, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = (x[rng.integers(0, n, 140)] + rng.standard_normal((140, dim)).astype(np.float32) * 0.05).astype(np.float32)[:nq]
    q[2] = rng.standard_normal(dim).astype(np.float32) * 1000.0
    q[3, 5], q[4, :], q[5, 7], q[6] = np.nan, np.inf, -np.inf, 0.0
    if poison:
        mins, maxs = x.min(0).copy(), x.max(0).copy() + 1e-3
        mins[3] = np.nan
        sq, ref = _quantizers(vg, ctx, x, (mins, maxs))
        codes = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    else:
        sq, ref = _quantizers(vg, ctx, x)
        codes = sq.encode(x)
    idx = _index(vg, ctx, sq, codes, metric)
    _on_equals_off(ctx, idx, [lambda: idx.search_sq8(q, k)])
    rescanned = idx.sq8_nomination_info()[2]
    assert rescanned == nq if poison else 3 <= rescanned <= 3 + nq // 20, rescanned   # the NaN and the two Inf queries, hardly any other
