"""vg_index_enable_int4_nomination with on & 4 (modes 5 and 6): vg_search_int4 batches under a row filter through the matrix-core
nomination — flat_gemm_int4_big_kernel's masked append above 128 queries, flat_gemm_int4_small_kernel's masked variants up to 128
(a batch filter: 64-row tiles skipped; per-query filters: the bit read behind the threshold) — against the masked numpy reference
(tests/int4_search_ref.py) and the search with the mode off, ids and score bits; every case asserts the GEMM scope and the mode."""
import ctypes
import functools

import numpy as np
import pytest

from tests import int4_search_ref as ref
from tests.test_gpu_int4_search import ctx, vg  # noqa: F401  (the module's fixtures)
from tests.test_gpu_int4_nomination import _index, nominate_always  # noqa: F401  (its helpers; VG_INT4_NOM_ALWAYS on)

pytestmark = pytest.mark.gpu
SMALL, BIG = "int4_codes_gemm_small", "int4_codes_gemm"   # the profile scopes of the two GEMMs on the nibble codes
SHORT = ("sparse", "sparse_q", "few")                     # filters under which every query's list is complete and at most 64 rows


@functools.lru_cache(maxsize=None)
def _data(n, dim):
    """clustered rows and 129 queries, once per shape"""
    rng = np.random.default_rng(n + dim)
    cent = rng.standard_normal((30, dim)).astype(np.float32) * 2
    x = (cent[rng.integers(0, 30, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.5).astype(np.float32)
    return x, (cent[rng.integers(0, 30, 129)] + rng.standard_normal((129, dim)).astype(np.float32) * 0.5).astype(np.float32)


def _masks(kind, rng, nq, n):
    """bool [n] (a batch filter) or [nq, n] (one per query)"""
    tile = np.arange(n) // 64
    if kind == "all":
        return np.ones(n, np.bool_)
    if kind == "tiles3":      # whole 64-row tiles empty: two of three, the first and the last among them; half of the others' rows
        return (tile % 3 == 1) & (tile != tile[-1]) & (rng.random(n) < 0.5)
    if kind in SHORT:   # 60 rows (~1 % of 8321) a filter: a list of at most 64 rows, a sample short of sel_k kept rows
        m = np.zeros((nq, n), np.bool_)
        for i in range(nq):
            m[i, rng.choice(n, 60, replace=False)] = True
        if kind == "few":           # ... and query 0 keeps 3 rows (fewer than k), query 1 none
            m[0], m[1] = False, False
            m[0, [5, n // 2, n - 1]] = True
        return m[0] if kind == "sparse" else m
    m = rng.random((nq, n)) < 0.4   # "batch40", "query40"
    return m[0] if kind == "batch40" else m


def _run(ctx, idx, q, k, masks, mode, scope):
    """the search with the mode off, then under `mode`: the reported mode, which of the two GEMM scopes ran, on == off"""
    off = idx.search_int4(q, k, mask=masks)
    idx.enable_int4_nomination(True, small_batches=mode == 6, filtered=True)
    assert idx.int4_nomination_info()[0] == mode
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SMALL), ctx.profile_read(BIG)
        on = idx.search_int4(q, k, mask=masks)
        ran = {s for s in (SMALL, BIG) if ctx.profile_read(s)[0] >= 1}
    finally:
        ctx.profile_enable(False)
    assert ran == {scope}, ran
    for qi in range(q.shape[0]):
        ref.assert_row(on[0][qi], on[1][qi], off[0][qi], off[1][qi], ("scan", qi))
    return on


def _check_reference(oq, codes, q, k, masks, got, queries):
    """the numpy reference over the rows a query's filter keeps (the others' scores are never looked at)"""
    for qi in queries:
        m = masks if masks.ndim == 1 else masks[qi]
        sc = np.zeros(codes.shape[0], np.float32)
        sc[m] = ref.row_scores(oq, q[qi], codes[m]) if m.any() else 0
        ref.assert_row(got[0][qi], got[1][qi], *ref.expected(sc, k, m), ("reference", qi))


# (queries, rows, dim, k, filter).  129 queries: the big tile; 7, 33, 100: one, two and four 32-query blocks of the small tile, the
# last one short; 100 at dim 640: two launches of two blocks.  8321 rows: above kFlatCap (4096), short last tiles; 4000: no sample.
CASES = [(129, 8321, 64, 10, "batch40"), (129, 8321, 96, 100, "query40"), (129, 4000, 64, 10, "few"), (129, 8321, 64, 100, "sparse_q"),
         (129, 8321, 96, 10, "all"), (7, 8321, 64, 10, "tiles3"), (7, 8321, 96, 10, "all"), (33, 8321, 96, 10, "query40"),
         (33, 8321, 64, 100, "few"), (33, 8321, 64, 10, "sparse"), (100, 8321, 64, 100, "batch40"), (100, 4000, 96, 10, "tiles3"),
         (100, 8321, 96, 100, "sparse_q"), (100, 4000, 640, 10, "query40")]


@pytest.mark.parametrize("nq,n,dim,k,kind", CASES)
def test_filtered_parity_with_reference_and_scan(vg, ctx, nq, n, dim, k, kind):
    x, q = _data(n, dim)
    q = q[:nq].copy()
    masks = _masks(kind, np.random.default_rng(nq + k), nq, n)
    idx, iq, oq, codes = _index(vg, ctx, x)
    codes[100:110] = codes[100]                                   # ties
    codes[200], codes[201], codes[n - 1] = 0x00, 0xFF, codes[7]   # an all-0 and an all-15 row; the last row equal to an early one
    q[2], q[3] = oq.decode(codes[100]), oq.decode(codes[n - 1])   # exactly decoded rows (one of the ten tied ones)
    if kind in SHORT and n > 4096:  # the premise, on the CPU: the sample (every 64th 128-row tile) keeps fewer than sel_k (8; 16) rows
        sampled = np.arange(n) // 128 % 64 == 0
        assert np.atleast_2d(masks)[:, sampled].sum(1).max() < (8 if k <= 48 else 16)
    idx.set_int4_codes(iq, codes)
    got = _run(ctx, idx, q, k, masks, 5 if nq > 128 else 6, BIG if nq > 128 else SMALL)
    _check_reference(oq, codes, q, k, masks, got, (0, 1, 2, 3, nq - 1))
    if kind in SHORT:               # no threshold: every kept row listed, a complete list the verify pair takes as it is
        assert idx.int4_nomination_info()[2] == 0, idx.int4_nomination_info()
    if kind == "few":               # fewer than k kept rows: the scan's padded answer
        assert got[0][0][3] == ref.INVALID_ID and got[0][1][0] == ref.INVALID_ID and np.isinf(got[1][1]).all()


def test_tied_scores_under_a_filter(vg, ctx):
    """every row four times: the k best are ties broken by row id, among the copies a query's filter keeps"""
    n, dim, k, nq = 4800, 64, 10, 40
    x, q = _data(n // 4, dim)
    idx, iq, oq, codes = _index(vg, ctx, np.tile(x, (4, 1)))
    masks = np.random.default_rng(9).random((nq, n)) < 0.5
    idx.set_int4_codes(iq, codes)
    _check_reference(oq, codes, q, k, masks, _run(ctx, idx, q[:nq], k, masks, 6, SMALL), (0, nq - 1))


def test_skipped_tiles_across_filter_windows(vg, ctx):
    """0.2 % kept of 600001 rows, 2344 tiles for 256 workgroups: a wave walks two filter windows, 88 % of its tiles skipped"""
    n, dim, k, nq = 600001, 64, 10, 100
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = x[rng.integers(0, n, nq)] + 0.05 * rng.standard_normal((nq, dim)).astype(np.float32)
    masks = rng.random(n) < 0.002
    masks[n - 1], q[0] = True, x[n - 1]
    idx, iq, oq, codes = _index(vg, ctx, x)
    idx.set_int4_codes(iq, codes)
    _check_reference(oq, codes, q, k, masks, _run(ctx, idx, q, k, masks, 6, SMALL), (0, 1, nq - 1))


def test_flag_values(vg, ctx):
    """4 is a flag without a mode and 7 is above 6: VG_ERR_INVALID_ARG (-1), the state as it was"""
    from vecgo_amd._lib import load
    idx, iq, oq, codes = _index(vg, ctx, _data(4000, 64)[0])
    idx.set_int4_codes(iq, codes)
    idx.enable_int4_nomination(True, small_batches=True)
    for bad in (4, 7):
        assert load().vg_index_enable_int4_nomination(idx._h, ctypes.c_int32(bad), None) == -1
        assert idx.int4_nomination_info()[0] == 2
