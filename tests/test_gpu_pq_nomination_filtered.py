"""vg_index_enable_pq_nomination_from_codes with on & 4 (modes 6 and 7): search_flat_filtered batches with scan = PQ over the whole
segment through the nomination from the codes — flat_gemm_codes_big_kernel's masked append above 128 queries,
flat_gemm_pq_small_kernel's masked variants up to 128 (a batch filter: a wave walks only the 64-row slices that keep a row; per-query
filters: the bit read behind the threshold) — against the oracle over the kept rows and the filtered scan with the flag off, ids and
score bits; every case asserts the GEMM scope and the mode."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests.test_gpu_pq_nomination_codes import _clustered_codes, _decoded, _mk, _random_pq, _same, bits, ctx, nominate_always, vg  # noqa: F401

pytestmark = pytest.mark.gpu
SMALL, BIG = "pq_codes_gemm_small", "pq_codes_gemm"   # the profile scopes of the two GEMMs on the PQ codes
SCANS = ("pq_adc_scan", "pq_adc_probe")               # ... and of the kernels a rescanned query takes
SHORT = ("sparse", "sparse_q", "few")                 # filters under which every query's list is complete and at most 64 rows
INVALID = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _data(n, m):
    """a quantizer, clustered codes with ties and extreme entries, 129 queries near decoded rows: once per shape"""
    rng = np.random.default_rng(n + m)
    opq = _random_pq(rng, 8 * m, m)
    codes = _clustered_codes(rng, n, m)
    codes[100:110] = codes[100]
    codes[200], codes[201], codes[n - 1] = 0, 255, codes[7]
    x = _decoded(opq, codes)
    q = (x[rng.integers(0, n, 129)] + rng.standard_normal((129, 8 * m)).astype(np.float32) * 0.05).astype(np.float32)
    q[2], q[3] = x[100], x[n - 1]   # exactly decoded rows (one of the ten tied ones; the last row, equal to an early one)
    return opq, codes, q


def _masks(kind, rng, nq, n):
    """bool [n] (a batch filter) or [nq, n] (one per query)"""
    tile = np.arange(n) // 64
    if kind == "all":
        return np.ones(n, np.bool_)
    if kind == "tiles3":      # whole 64-row slices empty: two of three, the first and the last among them; half of the others' rows
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
    idx.enable_pq_nomination_from_codes(False)
    off = idx.search_flat_filtered(q, k, masks, scan=1)
    idx.enable_pq_nomination_from_codes(True, small_batches=mode == 7, filtered=True)
    assert idx.pq_nomination_info()[0] == mode
    ctx.profile_enable(True)
    try:
        for s in (SMALL, BIG) + SCANS:
            ctx.profile_read(s)
        on = idx.search_flat_filtered(q, k, masks, scan=1)
        ran = {s for s in (SMALL, BIG) + SCANS if ctx.profile_read(s)[0] >= 1}
    finally:
        ctx.profile_enable(False)
    assert ran & {SMALL, BIG} == {scope}, ran
    assert _same(on, off)
    return on, ran


def _check_reference(opq, codes, q, k, masks, got, queries):
    """oracle.flat_search_pq over the rows a query's filter keeps (row order, so (score, row id) order, is preserved); padded behind them"""
    for qi in queries:
        rows = np.flatnonzero(masks if masks.ndim == 1 else masks[qi])
        eid, esc = o.flat_search_pq(opq, codes[rows], q[qi], k) if rows.size else (np.zeros(0, np.int64), np.zeros(0, np.float32))
        c = eid.size
        assert np.array_equal(got[0][qi, :c], rows[eid]) and np.array_equal(bits(got[1][qi, :c]), bits(esc)), qi
        assert (got[0][qi, c:] == INVALID).all() and np.isinf(got[1][qi, c:]).all(), qi


# (queries, rows, m, k, filter).  129 queries: the big tile; 33, 70, 100: two, three and four 32-query blocks of the small tile, the
# last one short; 97 at m = 96: two launches of two blocks.  8321 rows: above kFlatCap (4096), short last tile and slice; 4000: no
# sample.  m = 13, 17: rows at odd addresses, a zero granule; 17: a second chunk of one step, its last rows' read clamped.
CASES = [(129, 8321, 13, 10, "batch40"), (129, 8321, 24, 100, "query40"), (129, 4000, 17, 10, "few"), (129, 8321, 13, 100, "sparse_q"),
         (129, 8321, 24, 10, "all"), (33, 8321, 17, 10, "tiles3"), (33, 8321, 24, 10, "query40"), (33, 8321, 13, 100, "few"),
         (33, 8321, 13, 10, "sparse"), (70, 8321, 17, 100, "all"), (100, 8321, 13, 100, "batch40"), (100, 4000, 24, 10, "tiles3"),
         (100, 8321, 17, 100, "sparse_q"), (97, 4000, 96, 10, "query40")]


@pytest.mark.parametrize("nq,n,m,k,kind", CASES)
def test_filtered_parity_with_oracle_and_scan(vg, ctx, nominate_always, nq, n, m, k, kind):
    opq, codes, q = _data(n, m)
    q = q[:nq]
    masks = _masks(kind, np.random.default_rng(nq + k), nq, n)
    if kind in SHORT and n > 4096:  # the premise, on the CPU: the sample (every 64th 128-row tile) keeps fewer than sel_k (8; 16) rows
        sampled = np.arange(n) // 128 % 64 == 0
        assert np.atleast_2d(masks)[:, sampled].sum(1).max() < (8 if k <= 48 else 16)
    pq, idx = _mk(vg, ctx, opq, codes, n)
    got, ran = _run(ctx, idx, q, k, masks, 6 if nq > 128 else 7, BIG if nq > 128 else SMALL)
    _check_reference(opq, codes, q, k, masks, got, (0, 1, 2, nq - 1))
    if kind in SHORT:               # no threshold: every kept row listed, a complete list the verify pair takes as it is
        assert not ran & set(SCANS), ran
    if kind == "few":               # fewer than k kept rows: the scan's padded answer
        assert got[0][0][3] == INVALID and got[0][1][0] == INVALID and np.isinf(got[1][1]).all()


@pytest.mark.parametrize("small_grid", [0, 1])
def test_skipped_slices_across_filter_windows(vg, ctx, nominate_always, small_grid):
    """0.2 % kept of 300001 rows, 1172 tiles: about one 64-row slice in eight keeps a row; on 2 workgroups (VG_PQ_SMALL_GRID) a wave
    has 586 tiles in ten filter windows, the last one short"""
    n, m, k, nq = 300001, 4, 10, 40
    rng = np.random.default_rng(11)
    opq = _random_pq(rng, 8 * m, m)
    codes = _clustered_codes(rng, n, m)
    masks = rng.random(n) < 0.002
    masks[n - 1] = True
    x = _decoded(opq, codes[masks])
    q = (x[rng.integers(0, x.shape[0], nq)] + rng.standard_normal((nq, 8 * m)).astype(np.float32) * 0.05).astype(np.float32)
    q[0] = x[-1]
    pq, idx = _mk(vg, ctx, opq, codes, n)
    hooks.set_hook("VG_PQ_SMALL_GRID", small_grid)
    try:
        got, _ = _run(ctx, idx, q, k, masks, 7, SMALL)
    finally:
        hooks.set_hook("VG_PQ_SMALL_GRID", 0)
    _check_reference(opq, codes, q, k, masks, got, (0, 1, nq - 1))


def test_tied_scores_under_a_filter(vg, ctx, nominate_always):
    """every row four times: the k best are ties broken by row id, among the copies a query's filter keeps"""
    n, m, k, nq = 4800, 13, 10, 40
    opq, codes, q = _data(n // 4, m)
    codes = np.tile(codes, (4, 1))
    masks = np.random.default_rng(9).random((nq, n)) < 0.5
    pq, idx = _mk(vg, ctx, opq, codes, n)
    _check_reference(opq, codes, q, k, masks, _run(ctx, idx, q[:nq], k, masks, 7, SMALL)[0], (0, 2, nq - 1))


def test_flag_values(vg, ctx):
    """4 is a flag without a mode and 7 is above 6: VG_ERR_INVALID_ARG (-1), the state as it was; 5 is mode 6, and 0 frees it"""
    from vecgo_amd._lib import load
    opq, codes, q = _data(4000, 13)
    pq, idx = _mk(vg, ctx, opq, codes, 4000)
    idx.enable_pq_nomination_from_codes(True, small_batches=True)
    for bad in (4, 7):
        assert load().vg_index_enable_pq_nomination_from_codes(idx._h, ctypes.c_int32(bad), None) == -1
        assert idx.pq_nomination_info()[0] == 3
    held = idx.pq_nomination_info()[1]
    assert load().vg_index_enable_pq_nomination_from_codes(idx._h, ctypes.c_int32(5), None) == 0
    assert idx.pq_nomination_info() == (6, held)
    idx.enable_pq_nomination_from_codes(False)
    assert idx.pq_nomination_info() == (0, 0)
