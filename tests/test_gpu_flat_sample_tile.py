"""The flat search's threshold sample on the persistent 256 x 256 tile (flat_gemm_sample_big_kernel): above 128 queries, where
the nomination runs on the split tile, the sampled rows (every 64th 128-row tile) are scored by one bfloat16 product, a 256-row
tile being a PAIR of sampled 128-row tiles.  A wrong sample gives no wrong answer but a slow one, so every case here wants the
oracle's ids and score bits, the same from the same call under VG_FLAT_F32_SAMPLE (the fp32 128 x 128 sample), flat_stats()[0]
advanced by nq — and the planted cases count what was appended (flat_appended()).

The sampled tiles are rows [8192 j, 8192 j + 128); n = 4097 has one (the pair's second half is absent), 8193 two (the second
of one row), 8320 two whole, 16500 three (the second pair has one half, ragged), 24700 four (the last ragged)."""
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks

pytestmark = pytest.mark.gpu

HOOK = "VG_FLAT_F32_SAMPLE"
NS = (4097, 8193, 8320, 16500, 24700)
NQS = (129, 256, 257, 600)     # a ragged query tile, one whole, two and one query, three
DIMS = (32, 64, 96)            # one K step a tile (the prologue's S > 1 branches), two, three (the ring of three wraps)
KS = (1, 10, 16, 17, 48)       # 16 | 17: with and without the screen
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
    rng = np.random.default_rng(2000 + dim)
    return rng.standard_normal((NMAX, dim)).astype(np.float32), rng.standard_normal((NQMAX, dim)).astype(np.float32)


def both_ways(idx, search):
    """search() as the library runs it and under the hook: (result, (queries, exhaustive, retried, appended) deltas) of each"""
    out = []
    for on in (0, 1):
        hooks.set_hook(HOOK, on)
        try:
            s0, r0, a0 = idx.flat_stats(), idx.flat_retried(), idx.flat_appended()
            r = search()
            s1, r1, a1 = idx.flat_stats(), idx.flat_retried(), idx.flat_appended()
        finally:
            hooks.set_hook(HOOK, 0)
        out.append((r, (s1[0] - s0[0], s1[1] - s0[1], r1 - r0, a1 - a0)))
    return out


def same_scores(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def check(idx, search, nq, expect, what):
    """the conditions of every case: the oracle's ids and score bits, the same under the hook, flat_stats()[0] += nq"""
    got, ref = both_ways(idx, search)
    (ids, sc), st = got
    (hid, hsc), hst = ref
    assert np.array_equal(ids, hid), what
    assert same_scores(sc, hsc), what
    assert st[0] == nq and hst[0] == nq, (what, st, hst)
    for i in range(nq):
        eid, esc = expect(i)
        r = eid.size
        assert np.array_equal(ids[i, :r], eid), (what, i, ids[i], eid)
        assert same_scores(sc[i, :r], esc), (what, i)
    return got, ref


def run_shapes(vg, ctx, n, dim, metric, nqs, ks):
    rows, q = data(dim)
    exp = [o.flat_search_f32(rows[:n], dim, q[i], max(ks), metric) for i in range(max(nqs))]
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(rows[:n])
    try:
        for nq in nqs:
            for k in ks:
                check(idx, lambda: idx.search_flat(q[:nq], k), nq, lambda i: (exp[i][0][:k], exp[i][1][:k]), (n, dim, metric, nq, k))
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", NS)
def test_sample_tile_matches_oracle_and_fp32_sample(vg, ctx, n, dim, metric):
    run_shapes(vg, ctx, n, dim, metric, NQS, KS)


@pytest.mark.parametrize("metric", [0, 2])
def test_sample_tile_dim_768(vg, ctx, metric):
    """the benchmark's row length: 24 K steps a tile"""
    run_shapes(vg, ctx, 16500, 768, metric, (257,), (10, 17))


def test_last_chunk_of_at_most_128_queries(vg, ctx):
    """One call of 4096 + 100 queries: the first chunk (16 query tiles, four and more tiles per workgroup) samples on the
    persistent tile, the second (100 queries: the 32-row tiles, no split tile) keeps its fp32 sample."""
    n, dim, k, nq = 8320, 32, 10, 4196
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(rows)
    try:
        check(idx, lambda: idx.search_flat(q, k), nq, lambda i: o.flat_search_f32(rows, dim, q[i], k), "two chunks")
    finally:
        idx.close()


# ---- planted rows ---------------------------------------------------------------------------------------------------------
# The centre c has |c| = 1 (every component +-1/8, dim 64); a query is c with at most one component moved by 2^-7 (within 0.01
# of c); planted row number j is c + (1 + j) e along an axis of its own, so its score |x|^2 - 2 q.x is (1 + j)^2 - 1 up to 0.02
# (1 + j): at least 3 from its neighbours'; every other row is standard normal around a point 40 away.  All components of the
# planted rows and of the queries are multiples of 2^-7 of at most 8 significant bits: bfloat16 holds them, every product is a
# multiple of 2^-10 and every partial sum of a row's score is exact in fp32 in ANY order.  That is what makes the appended count
# exact: the threshold is the 8th best score of the sample, the nomination GEMM scores that same row again, and "below the
# threshold" must not depend on the order in which two kernels add the same products (equal scores: not appended).
PLANT_N, PLANT_DIM = 24700, 64
TILES = (0, 8192, 16384, 24576)


def inside(r):
    return any(t <= r < t + 128 for t in TILES)


def bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def planted(order, nq, seed):
    """rows [PLANT_N, PLANT_DIM], queries [nq, PLANT_DIM]: row order[j] is the j-th nearest of every query.  Asserts on the CPU
    that a model of the bfloat16 sample (both operands rounded to nearest even, fp32 dot product, |x|^2 - 2 q.x) ranks the
    planted rows as fp64 does, neighbours further apart than twice the model's largest error, every other row beyond them."""
    assert len(order) <= 31 and len(set(order)) == len(order)
    rng = np.random.default_rng(seed)
    c = (rng.integers(0, 2, PLANT_DIM) * 2 - 1).astype(np.float32) / 8
    w = rng.standard_normal(PLANT_DIM)
    rows = (c + 40.0 * w / np.linalg.norm(w) + rng.standard_normal((PLANT_N, PLANT_DIM))).astype(np.float32)
    axes = rng.permutation(PLANT_DIM)
    for j, r in enumerate(order):
        rows[r] = c
        rows[r, axes[j]] += np.sign(c[axes[j]]) * (1 + j)
    q = np.tile(c, (nq, 1))
    for i in range(nq):
        m = i % (2 * PLANT_DIM + 1)
        if m:
            q[i, (m - 1) // 2] += (1 if m % 2 else -1) / 128
    assert np.abs(q - c).max() < 0.01 and abs(float(np.linalg.norm(c.astype(np.float64))) - 1) < 1e-6
    qu = q[:2 * PLANT_DIM + 1]                         # the distinct queries
    exact = (rows.astype(np.float64) ** 2).sum(1)[None, :] - 2 * qu.astype(np.float64) @ rows.astype(np.float64).T
    dots = bf16_rne(qu) @ bf16_rne(rows).T             # fp32
    model = ((rows * rows).sum(1, dtype=np.float32)[None, :] - 2 * dots).astype(np.float64)
    err = np.abs(model[:, order] - exact[:, order]).max()
    gap = np.diff(exact[:, order], axis=1).min()
    assert np.all(np.diff(model[:, order], axis=1) > 0) and gap >= 3 - 0.02 * 2 * len(order) and gap > 2 * err, (gap, err)
    rest = np.setdiff1d(np.arange(PLANT_N), order)
    assert model[:, rest].min() > model[:, order].max() + 100 and exact[:, rest].min() > exact[:, order].max() + 100
    return rows, q


def appended_model(order, kept):
    """how many rows a query appends: its threshold is the score of the 8th nearest KEPT row of the sampled tiles, and what is
    appended are the kept rows strictly nearer than that one (kept: the ranks its filter lets through)"""
    ranks = [j for j in kept if inside(order[j])]
    assert len(ranks) >= 8
    return sum(1 for j in kept if j < ranks[7])


def test_nearest_rows_inside_both_halves_of_both_pairs(vg, ctx):
    """The 10 nearest rows lie in the sampled tiles, in both halves of both pairs, first of all the halves' first and last rows
    (the second pair's second half is ragged: 24699 is the segment's last row).  The 8th best of the sample is the threshold:
    exactly the 7 nearest rows are appended for every query, and k = 5 is answered by the screen (scores 24 and 63 against a
    margin of ~14) with no fall-back and no retry."""
    order = [0, 8319, 16384, 24699, 127, 8192, 16511, 24576, 1, 16400]
    nq, k = 257, 5
    rows, q = planted(order, nq, 41)
    assert all(inside(r) for r in order) and appended_model(order, range(len(order))) == 7
    idx = vg.Index(ctx, PLANT_N, PLANT_DIM)
    idx.set_vectors(rows)
    try:
        got, ref = check(idx, lambda: idx.search_flat(q, k), nq, lambda i: o.flat_search_f32(rows, PLANT_DIM, q[i], k), "inside")
        assert got[0][0].tolist() == [order[:k]] * nq
        assert got[1] == (nq, 0, 0, 7 * nq), got[1]
        assert ref[1] == (nq, 0, 0, 7 * nq), ref[1]
    finally:
        idx.close()


def test_nearest_rows_alternate_across_the_sampled_tiles_edges(vg, ctx):
    """The nearest rows alternate outside | inside the sampled tiles across their edges (8191 | 8192, 8319 | 8320, 16383 |
    16384, 127 | 128, 24575 | 24576): the sample sees every other one.  Its 8th best is planted row number 15, so exactly the
    15 nearer rows are appended, from both sides of the edges, and k = 10 (scores 99 and 255) is answered without a fall-back."""
    order = [8191, 8192, 8320, 8319, 16383, 16384, 128, 127, 8190, 8193, 16385 + 127, 16385, 24575, 24576, 129, 0, 16511, 1]
    nq, k = 257, 10
    rows, q = planted(order, nq, 42)
    assert [inside(r) for r in order[:16]] == [False, True] * 8 and appended_model(order, range(len(order))) == 15
    idx = vg.Index(ctx, PLANT_N, PLANT_DIM)
    idx.set_vectors(rows)
    try:
        got, ref = check(idx, lambda: idx.search_flat(q, k), nq, lambda i: o.flat_search_f32(rows, PLANT_DIM, q[i], k), "edges")
        assert got[0][0].tolist() == [order[:k]] * nq
        assert got[1][1] == 0 and got[1][3] == 15 * nq, got[1]
        assert ref[1][1] == 0 and ref[1][3] == 15 * nq, ref[1]
    finally:
        idx.close()


def test_filter_rejects_every_other_planted_row(vg, ctx):
    """search_flat_filtered, one filter per query: query i's filter rejects the planted rows of rank i % 2, i % 2 + 2, ... and
    a random third of the other rows.  A rejected row is +Inf in the sample — it does not count towards the 8th best — and is
    not appended: the appended count is what the kept rows give."""
    ins = [8192, 8319, 16384, 127, 8193, 16385, 24576, 0, 1, 16511, 24699, 8200, 16400, 24600, 2, 126, 8318, 16510, 24577, 3]
    outs = [8191, 8320, 16383, 128, 8190, 16512, 24575, 129, 8321, 16382]
    order = [outs.pop(0) if j % 3 == 2 else ins.pop(0) for j in range(30)]
    nq, k = 257, 10
    rows, q = planted(order, nq, 43)
    rng = np.random.default_rng(5)
    mask = rng.random((nq, PLANT_N)) > 1.0 / 3.0
    kept = [[j for j in range(len(order)) if j % 2 != i % 2] for i in range(nq)]
    for i in range(nq):
        mask[i, order] = False
        mask[i, [order[j] for j in kept[i]]] = True
    want = sum(appended_model(order, kept[i]) for i in range(nq))
    seg = o.FlatSegment(rows, PLANT_DIM)
    idx = vg.Index(ctx, PLANT_N, PLANT_DIM)
    idx.set_vectors(rows)
    try:
        got, ref = check(idx, lambda: idx.search_flat_filtered(q, k, mask, 0, scan=idx.SCAN_F32), nq,
                         lambda i: seg.search(q[i], k, mask=mask[i]), "filter")
        assert got[0][0].tolist() == [[order[j] for j in kept[i][:k]] for i in range(nq)]
        assert got[1][3] == want and ref[1][3] == want, (got[1], ref[1], want)
    finally:
        idx.close()


# ---- values bfloat16 cannot hold ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("bad", [np.inf, np.nan, 3e38])
def test_non_finite_row_in_a_sampled_tile_and_query(vg, ctx, bad, metric):
    """One row of a sampled tile holds Inf, NaN or 3e38 (which bfloat16 rounds to Inf) and one query an Inf: the sample's scores
    for them are Inf or NaN, no proof holds on a segment whose largest norm is not finite, and the exhaustive kernel or the
    heap replay answers — the oracle's results (NaN == NaN)."""
    n, dim, nq, k = 8320, 64, 130, 10
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    rows[8200, 5] = bad
    q[7, 3] = np.inf
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(rows)
    try:
        check(idx, lambda: idx.search_flat(q, k), nq, lambda i: o.flat_search_f32(rows, dim, q[i], k, metric=metric), (bad, metric))
    finally:
        idx.close()
