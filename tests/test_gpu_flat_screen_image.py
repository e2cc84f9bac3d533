"""The compact hi-only query image of the flat search's screen (flat_split_queries_kernel writes it beside the hi | lo image; the
screen and the threshold sample on its tile, flat_gemm_big_body under OPS = kBigScreen, fill their query tiles from it: two
LDS-DMA pieces of 16 rows x 64 B per wave and K step, rows XOR-swizzled four to a bank window).  The image changes no product and
no order: every case wants the oracle's ids and score bits, the same from the same call under VG_FLAT_NO_SCREEN (the split tile
for every tile, from the hi | lo image — its sample still reads the new one), and flat_stats()[0] advanced by nq.

Shapes, the smallest that reach each seam: nq 129 (a ragged single tile: the image's rows past nq are the last query), 256 (a
whole tile), 257 (a second tile of one query), 600 (several); dim 32 / 64 / 96 (one, two, three K steps a tile: the ring of
three row buffers wraps, the two query buffers alternate on an odd count) and 768 once; n 300 (at most 4096 rows: no sample,
thresholds from flat_thr_cap_kernel), 4097 and 8320 (one sampled tile and a pair), 16500 (a ragged last row tile); k 1, 10, 16
(the screen) and 17 (no screen, but the sample still reads the new image); both metrics."""
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks

pytestmark = pytest.mark.gpu

HOOK = "VG_FLAT_NO_SCREEN"
NS = (300, 4097, 8320, 16500)
NQS = (129, 256, 257, 600)
DIMS = (32, 64, 96)
KS = (1, 10, 16, 17)
KMAX, NQMAX, NMAX = max(KS), max(NQS), max(NS)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


@functools.lru_cache(maxsize=None)
def data(dim):
    """rows [NMAX, dim] and queries [NQMAX, dim]: every n takes the first n rows, every nq the first nq queries"""
    rng = np.random.default_rng(7100 + dim)
    return rng.standard_normal((NMAX, dim)).astype(np.float32), rng.standard_normal((NQMAX, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def expected(n, dim, metric, nq=NQMAX, k=KMAX):
    """the oracle's KMAX best of the first nq queries over the first n rows, computed once and shared"""
    rows, q = data(dim)
    return [o.flat_search_f32(rows[:n], dim, q[i], k, metric) for i in range(nq)]


def counted(idx, search, hook=None):
    """search() (under a hook): (result, deltas of (queries, exhaustive, retried, appended))"""
    if hook:
        hooks.set_hook(hook, 1)
    try:
        s0, r0, a0 = idx.flat_stats(), idx.flat_retried(), idx.flat_appended()
        r = search()
        s1, r1, a1 = idx.flat_stats(), idx.flat_retried(), idx.flat_appended()
    finally:
        if hook:
            hooks.set_hook(hook, 0)
    return r, (s1[0] - s0[0], s1[1] - s0[1], r1 - r0, a1 - a0)


def same_scores(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def check(idx, search, nq, k, exp, what, checked=None):
    """the conditions of every case: the oracle's ids and score bits (for the queries `checked`: default all), the same under
    the hook for every query, flat_stats()[0] += nq both ways"""
    (ids, sc), st = counted(idx, search)
    (hid, hsc), hst = counted(idx, search, HOOK)
    assert np.array_equal(ids, hid), what
    assert same_scores(sc, hsc), what
    assert st[0] == nq and hst[0] == nq, (what, st, hst)
    for i in (range(nq) if checked is None else checked):
        eid, esc = exp(i)
        eid, esc = eid[:k], esc[:k]
        assert np.array_equal(ids[i, :eid.size], eid), (what, i, ids[i], eid)
        assert same_scores(sc[i, :eid.size], esc), (what, i)
    return st, hst


def open_index(vg, ctx, n, dim, metric):
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(data(dim)[0][:n])
    return idx


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", NS)
def test_image_matches_oracle_and_split_tile(vg, ctx, n, dim, metric):
    q = data(dim)[1]
    exp = expected(n, dim, metric)
    idx = open_index(vg, ctx, n, dim, metric)
    try:
        for nq in NQS:
            for k in KS:
                check(idx, lambda: idx.search_flat(q[:nq], k), nq, k, lambda i: exp[i], (n, dim, metric, nq, k))
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_image_dim_768(vg, ctx, metric):
    """the benchmark's row length, 24 K steps a tile, with a second tile of one query"""
    n, dim, nq = 16500, 768, 257
    q = data(dim)[1]
    exp = expected(n, dim, metric, nq)
    idx = open_index(vg, ctx, n, dim, metric)
    try:
        for k in (10, 17):
            check(idx, lambda: idx.search_flat(q[:nq], k), nq, k, lambda i: exp[i], (n, dim, metric, k))
    finally:
        idx.close()


def test_one_call_spanning_two_chunks(vg, ctx):
    """4096 + 130 queries: the first chunk's image is 16 whole tiles (four and more tiles per workgroup), the second chunk's a
    ragged one of 130 queries written over its first tile.  Every 37th query against the oracle, every query against the split
    tile."""
    n, dim, k, nq = 4097, 32, 10, 4096 + 130
    rng = np.random.default_rng(4227)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(rows)
    try:
        check(idx, lambda: idx.search_flat(q, k), nq, k, lambda i: o.flat_search_f32(rows, dim, q[i], k), "two chunks", range(0, nq, 37))
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_every_query_retried_from_the_hi_lo_image(vg, ctx, metric):
    """VG_FLAT_SCREEN_FAIL: every screen proof counts as failed and every query is nominated again on the split tile, which reads
    the hi | lo image written beside the compact one in the same launch: the oracle's results, flat_retried() += nq"""
    n, dim, nq, k = 8320, 96, 257, 10
    q = data(dim)[1]
    exp = expected(n, dim, metric)
    idx = open_index(vg, ctx, n, dim, metric)
    try:
        (ids, sc), st = counted(idx, lambda: idx.search_flat(q[:nq], k), "VG_FLAT_SCREEN_FAIL")
        assert st[0] == nq and st[1] == 0 and st[2] == nq, st
        for i in range(nq):
            assert np.array_equal(ids[i], exp[i][0][:k]) and same_scores(sc[i], exp[i][1][:k]), i
    finally:
        idx.close()


# flat_appended() of one search_flat call of the first 600 queries of data(dim) over its first n rows, L2, as a build of the
# commit BEFORE the compact image reports it (that commit's library, this file's data; k = 10: the screen's lists, k = 17: the
# split tile's behind the sample).  A candidate is appended where its score is below its query's threshold: equal counts are what
# "the same score bits" means at the kernels' output, the sample's (the thresholds) and the screen's (the compares) alike.
PARENT_APPENDED = {
    (4097, 32, 10): 147542,
    (4097, 32, 17): 147735,
    (8320, 32, 10): 150607,
    (8320, 32, 17): 150713,
    (16500, 32, 10): 201252,
    (16500, 32, 17): 201387,
    (4097, 64, 10): 137515,
    (4097, 64, 17): 137591,
    (8320, 64, 10): 133606,
    (8320, 64, 17): 133716,
    (16500, 64, 10): 185620,
    (16500, 64, 17): 185754,
    (4097, 96, 10): 163983,
    (4097, 96, 17): 163998,
    (8320, 96, 10): 167239,
    (8320, 96, 17): 167288,
    (16500, 96, 10): 231619,
    (16500, 96, 17): 231710,
}


@pytest.mark.parametrize("dim", DIMS)
def test_appended_counts_are_the_previous_kernels(vg, ctx, dim):
    q = data(dim)[1]
    for n in NS[1:]:
        idx = open_index(vg, ctx, n, dim, 0)
        try:
            for k in (10, 17):
                _, st = counted(idx, lambda: idx.search_flat(q, k))
                assert st[0] == NQMAX and st[3] == PARENT_APPENDED[(n, dim, k)], ((n, dim, k), st)
        finally:
            idx.close()
