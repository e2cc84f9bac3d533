"""vg_index_enable_sq8_nomination_from_codes with on & 4 (modes 6 and 7): search_flat_filtered batches with scan = SQ8 over the whole
segment through the nomination from the codes — flat_gemm_sq8_big_kernel's masked append above 128 queries,
flat_gemm_sq8_small_kernel's masked variants up to 128 (a batch filter: a wave loads only the 64-row code tiles that keep a row;
per-query filters: the bit read behind the threshold) — against the oracle over the kept rows and the filtered scan with the flag
off, ids and score bits, L2 and Dot; every case asserts the GEMM scope and the mode."""
import ctypes
import functools

import numpy as np
import pytest

from tests import hooks
from tests.test_gpu_sq8_nomination_codes import DOT, L2, _index, _oracle, _quantizers, _same, bits, ctx, nominate_always, vg  # noqa: F401

pytestmark = pytest.mark.gpu
SMALL, BIG = "sq8_codes_gemm_small", "sq8_codes_gemm"   # the profile scopes of the two GEMMs on the code tiles
SCANS = ("sq8_scan", "sq8_probe")                       # ... and of the kernels a rescanned query takes
SHORT = ("sparse", "sparse_q", "few")                   # filters under which every query's list is complete and at most 64 rows
INVALID = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _data(n, dim):
    """clustered rows with ties and extreme codes, 129 queries near rows: once per shape (the quantizer's parameters follow from x)"""
    rng = np.random.default_rng(n + dim)
    cent = rng.standard_normal((30, dim)).astype(np.float32) * 2
    x = (cent[rng.integers(0, 30, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.5).astype(np.float32)
    q = (x[rng.integers(0, n, 129)] + rng.standard_normal((129, dim)).astype(np.float32) * 0.05).astype(np.float32)
    return x, q


def _mk(vg, ctx, x, metric, plant=True):
    """the quantizers, the codes (ties, an all-0 and an all-255 row, the last row equal to an early one) and the index"""
    sq, ref = _quantizers(vg, ctx, x)
    codes = sq.encode(x)
    if plant:
        n = codes.shape[0]
        codes[100:110] = codes[100]
        codes[200], codes[201], codes[n - 1] = 0, 255, codes[7]
    return ref, codes, _index(vg, ctx, sq, codes, metric)


def _masks(kind, rng, nq, n):
    """bool [n] (a batch filter) or [nq, n] (one per query)"""
    tile = np.arange(n) // 64
    if kind == "all":
        return np.ones(n, np.bool_)
    if kind == "tiles3":      # whole 64-row code tiles empty: two of three, the first and the last among them; half of the others' rows
        return (tile % 3 == 1) & (tile != tile[-1]) & (rng.random(n) < 0.5)
    if kind in SHORT:         # 60 rows a filter: a list of at most 64 rows, a sample short of sel_k kept rows
        m = np.zeros((nq, n), np.bool_)
        for i in range(nq):
            m[i, rng.choice(n, 60, replace=False)] = True
        if kind == "few":     # ... and query 0 keeps 3 rows (fewer than k), query 1 none
            m[0], m[1] = False, False
            m[0, [5, n // 2, n - 1]] = True
        return m[0] if kind == "sparse" else m
    m = rng.random((nq, n)) < 0.4   # "batch40", "query40"
    return m[0] if kind == "batch40" else m


def _run(ctx, idx, q, k, masks, mode, scope):
    """the filtered scan with the mode off, then under `mode`: the reported mode, which scopes ran, on == off; (result, scopes)"""
    idx.enable_sq8_nomination_from_codes(False)
    off = idx.search_flat_filtered(q, k, masks, scan=idx.SCAN_SQ8)
    idx.enable_sq8_nomination_from_codes(True, small_batches=mode == 7, filtered=True)
    assert idx.sq8_nomination_info()[0] == mode
    ctx.profile_enable(True)
    try:
        for s in (SMALL, BIG) + SCANS:
            ctx.profile_read(s)
        on = idx.search_flat_filtered(q, k, masks, scan=idx.SCAN_SQ8)
        ran = {s for s in (SMALL, BIG) + SCANS if ctx.profile_read(s)[0] >= 1}
    finally:
        ctx.profile_enable(False)
    assert ran & {SMALL, BIG} == {scope}, ran
    assert _same(on, off)
    return on, ran


def _check_reference(ref, x, codes, metric, q, k, masks, got, queries):
    """the oracle over the rows a query's filter keeps (row order, so (score, row id) order, is preserved); padded behind them"""
    for qi in queries:
        rows = np.flatnonzero(masks if masks.ndim == 1 else masks[qi])
        eid, esc = _oracle(ref, x[rows], codes[rows], metric, q[qi], k) if rows.size else (np.zeros(0, np.int64), np.zeros(0, np.float32))
        c = eid.size
        assert np.array_equal(got[0][qi, :c], rows[eid]) and np.array_equal(bits(got[1][qi, :c]), bits(esc)), qi
        assert (got[0][qi, c:] == INVALID).all() and np.isinf(got[1][qi, c:]).all(), qi


# (queries, rows, dim, k, filter, metric).  129 queries: the big tile; 33, 70, 100: two, three and four 32-query blocks of the small
# tile, the last one short; 97 at dim 768: two launches of two blocks.  8321 rows: above kFlatCap (4096), so a sample; the last row
# tile (rows 8192 ..) has two whole code tiles, one of a single row and one past the codes.  4000: no sample, everything appended.
# dim 16: one group, lane half 1 has none; 100: 7 groups, the last partial; 128; 768.
CASES = [(129, 8321, 16, 10, "batch40", DOT), (129, 8321, 128, 100, "query40", L2), (129, 4000, 100, 10, "few", L2),
         (129, 8321, 16, 100, "sparse_q", L2), (129, 8321, 128, 10, "all", L2), (33, 8321, 100, 10, "tiles3", L2),
         (33, 8321, 100, 10, "tiles3", DOT), (33, 8321, 128, 10, "query40", L2), (33, 8321, 16, 100, "few", L2),
         (33, 4000, 128, 10, "few", DOT), (33, 8321, 16, 10, "sparse", L2), (70, 8321, 100, 100, "all", L2),
         (100, 8321, 16, 100, "batch40", L2), (100, 4000, 128, 10, "tiles3", L2), (100, 8321, 100, 100, "sparse_q", DOT),
         (97, 4000, 768, 10, "query40", L2)]


@pytest.mark.parametrize("nq,n,dim,k,kind,metric", CASES)
def test_filtered_parity_with_oracle_and_scan(vg, ctx, nominate_always, nq, n, dim, k, kind, metric):
    x, q = _data(n, dim)
    q = q[:nq].copy()
    masks = _masks(kind, np.random.default_rng(nq + k), nq, n)
    if kind in SHORT and n > 4096:  # the premise, on the CPU: the sample (every 64th 128-row tile) keeps fewer than sel_k (8; 16) rows
        sampled = np.arange(n) // 128 % 64 == 0
        assert np.atleast_2d(masks)[:, sampled].sum(1).max() < (8 if k <= 48 else 16)
    ref, codes, idx = _mk(vg, ctx, x, metric)
    q[2], q[3] = ref.decode(codes[100]), ref.decode(codes[n - 1])   # exactly rows: one of the ten tied ones; the last, equal to an early one
    got, ran = _run(ctx, idx, q, k, masks, 6 if nq > 128 else 7, BIG if nq > 128 else SMALL)
    _check_reference(ref, x, codes, metric, q, k, masks, got, (0, 1, 2, 3, nq - 1))
    if kind in SHORT:               # no threshold: every kept row listed, a complete list the verify pair takes as it is
        assert not ran & set(SCANS), ran
    if kind == "few":               # fewer than k kept rows: the scan's padded answer
        assert got[0][0][3] == INVALID and got[0][1][0] == INVALID and np.isinf(got[1][1]).all()


@pytest.mark.parametrize("small_grid", [0, 1])
def test_skipped_tiles_across_filter_windows(vg, ctx, nominate_always, small_grid):
    """0.2 % kept of 300001 rows, 1172 row tiles: about one 64-row code tile in eight keeps a row.  A filter window is 64 of a wave's
    tiles (kSliceWindow): on 2 workgroups (VG_SQ8_SMALL_GRID) a wave has 586 tiles = nine whole windows and a tenth of 10 tiles, and
    its stream of live tiles crosses all of them; the last row (in the last, short code tile) is kept and query 0 equals it"""
    n, dim, k, nq = 300001, 32, 10, 40
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    masks = rng.random(n) < 0.002
    masks[n - 1] = True
    ref, codes, idx = _mk(vg, ctx, x, L2, plant=False)
    kept = np.flatnonzero(masks)
    q = (x[kept[rng.integers(0, kept.size, nq)]] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.05).astype(np.float32)
    q[0] = ref.decode(codes[n - 1])
    hooks.set_hook("VG_SQ8_SMALL_GRID", small_grid)
    try:
        got, _ = _run(ctx, idx, q, k, masks, 7, SMALL)
    finally:
        hooks.set_hook("VG_SQ8_SMALL_GRID", 0)
    _check_reference(ref, x, codes, L2, q, k, masks, got, (0, 1, nq - 1))
    assert got[0][0][0] == n - 1


def test_tied_scores_under_a_filter(vg, ctx, nominate_always):
    """every row four times: the k best are ties broken by row id, among the copies a query's filter keeps"""
    n, dim, k, nq = 4800, 100, 10, 40
    x, q = _data(n // 4, dim)
    x = np.tile(x, (4, 1))
    masks = np.random.default_rng(9).random((nq, n)) < 0.5
    ref, codes, idx = _mk(vg, ctx, x, L2, plant=False)
    _check_reference(ref, x, codes, L2, q, k, masks, _run(ctx, idx, q[:nq], k, masks, 7, SMALL)[0], (0, 2, nq - 1))


def test_flag_values(vg, ctx):
    """4 is a flag without a mode and 7 is above 6: VG_ERR_INVALID_ARG (-1), the state as it was; 5 is mode 6, and 0 frees it"""
    from vecgo_amd._lib import load
    ref, codes, idx = _mk(vg, ctx, _data(4000, 16)[0], L2)
    idx.enable_sq8_nomination_from_codes(True, small_batches=True)
    for bad in (4, 7):
        assert load().vg_index_enable_sq8_nomination_from_codes(idx._h, ctypes.c_int32(bad), None) == -1
        assert idx.sq8_nomination_info()[0] == 3
    held = idx.sq8_nomination_info()[1]
    assert load().vg_index_enable_sq8_nomination_from_codes(idx._h, ctypes.c_int32(5), None) == 0
    assert idx.sq8_nomination_info()[:2] == (6, held)
    idx.enable_sq8_nomination_from_codes(False)
    assert idx.sq8_nomination_info() == (0, 0, 0)
