"""The flat search scores its sampled row tiles once: the rows of every 64th 128-row tile that pass a query's threshold are
appended from the sample's scores (flat_sample_append_kernel) and the main GEMM leaves those tiles out (GemmArgs::skip_stride).
Every result here is compared with the oracle's flat scan AND with the same call under VG_FLAT_RESCORE_SAMPLE (the main GEMM
multiplies every tile, no append from the sample): ids, score bits and the flat_stats() counters must be the same.

The sample exists for n > 4096; the sampled tiles are rows [8192 j, 8192 j + 128).  A lost sampled row is a missing
candidate, a row appended by both kernels a doubled one: the planted cases put the nearest rows there."""
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks

pytestmark = pytest.mark.gpu

HOOK = "VG_FLAT_RESCORE_SAMPLE"
NS = (4097, 8192, 8193, 8250, 8320, 8321, 16500)   # one sampled tile .. three, the last one of 1 row / ragged
NQS = (5, 64, 96, 97, 128, 130, 257)               # the 32-row tiles (no skipping there); the 128-tile, whole and ragged
DIMS = (64, 100, 70)                               # LDS-DMA kernel, its ragged K edge, the register-staged kernel
KS = (1, 10, 48)
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
    rng = np.random.default_rng(1000 + dim)
    return rng.standard_normal((NMAX, dim)).astype(np.float32), rng.standard_normal((NQMAX, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(n, dim, metric):
    """the oracle's KMAX best of every query, computed once: its k best are the first k of them ((score, row id) is a total order)"""
    rows, q = data(dim)
    return [o.flat_search_f32(rows[:n], dim, q[i], KMAX, metric) for i in range(NQMAX)]


def both_ways(idx, search):
    """search() as the library runs it and under the hook: ((ids, scores), stats delta) of each"""
    out = []
    for on in (0, 1):
        hooks.set_hook(HOOK, on)
        try:
            s0 = idx.flat_stats()
            r = search()
            s1 = idx.flat_stats()
        finally:
            hooks.set_hook(HOOK, 0)
        out.append((r, (s1[0] - s0[0], s1[1] - s0[1])))
    return out


def same_as_hook(got, ref, what):
    (ids, sc), st = got
    (hid, hsc), hst = ref
    assert np.array_equal(ids, hid), what
    assert np.array_equal(bits(sc), bits(hsc)), what
    assert st == hst, (what, st, hst)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", NS)
def test_sample_scored_once_matches_oracle_and_rescore(vg, ctx, n, dim, metric):
    rows, q = data(dim)
    exp = reference(n, dim, metric)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(rows[:n])
    try:
        for nq in NQS:
            for k in KS:
                got, ref = both_ways(idx, lambda: idx.search_flat(q[:nq], k))
                same_as_hook(got, ref, (nq, k))
                assert got[1][0] == nq
                ids, sc = got[0]
                for i in range(nq):
                    eid, esc = exp[i]
                    assert np.array_equal(ids[i], eid[:k]), (nq, k, i, ids[i], eid[:k])
                    assert np.array_equal(bits(sc[i]), bits(esc[:k])), (nq, k, i)
    finally:
        idx.close()


# ---- planted rows ---------------------------------------------------------------------------------------------------------
# Queries sit within 0.01 of a centre c; planted row number j is c + (1 + j / 8) * u_j with |u_j| = 1, so planted rows are
# nearer than every other row (standard normal around 3 c / |c| * 20: tens of units away) and their L2 scores are spaced by
# about (1 + j / 8)^2 steps of 0.25 and more — far above the rounding of a 64-term fp32 dot product (~1e-5 here).
PLANT_N, PLANT_DIM = 16500, 64
INSIDE = list(range(0, 128)) + list(range(8192, 8320))   # rows of the sampled tiles 0 and 64 (tile 128 stays random)


def planted(order, nq, seed):
    """rows [PLANT_N, PLANT_DIM], queries [nq, PLANT_DIM]: row order[j] is the j-th nearest of every query"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal(PLANT_DIM).astype(np.float32)
    rows = (rng.standard_normal((PLANT_N, PLANT_DIM)) + 20.0 * c / np.linalg.norm(c) * 3.0).astype(np.float32)
    u = rng.standard_normal((len(order), PLANT_DIM))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for j, r in enumerate(order):
        rows[r] = (c + (1.0 + j / 8.0) * u[j]).astype(np.float32)
    q = (c + 0.01 * rng.standard_normal((nq, PLANT_DIM))).astype(np.float32)
    return rows, q


def check_planted(vg, ctx, rows, q, k, search=None, expect=None):
    idx = vg.Index(ctx, rows.shape[0], rows.shape[1])
    idx.set_vectors(rows)
    try:
        run = (lambda: idx.search_flat(q, k)) if search is None else (lambda: search(idx))
        got, ref = both_ways(idx, run)
        same_as_hook(got, ref, k)
        ids, sc = got[0]
        for i in range(q.shape[0]):
            eid, esc = expect(i) if expect else o.flat_search_f32(rows, rows.shape[1], q[i], k)
            r = eid.size
            assert np.array_equal(ids[i, :r], eid), (i, ids[i], eid)
            assert np.array_equal(bits(sc[i, :r]), bits(esc)), i
        return got, ref
    finally:
        idx.close()


@pytest.mark.parametrize("k", [5, 10, 48])
def test_nearest_rows_all_inside_sampled_tiles(vg, ctx, k):
    """The 256 nearest rows of every query are exactly the rows of the sampled tiles 0 and 64, the tiles' first and last rows
    (0, 127, 8192, 8319) the nearest of all.  The threshold is the 8th best of the sample, so the 7 nearest rows pass it and
    nothing else does: k = 5 is answered from the appended sample alone (no fall-back: the 5th and the 8th score are 0.4
    apart), k >= 8 cannot be proven from 7 candidates and falls back — as under the hook."""
    rng = np.random.default_rng(3)
    rest = [r for r in INSIDE if r not in (0, 127, 8192, 8319)]
    order = [8192, 0, 8319, 127] + [int(r) for r in rng.permutation(rest)]
    rows, q = planted(order, 130, 31)
    got, ref = check_planted(vg, ctx, rows, q, k)
    assert got[0][0][:, :4].tolist() == [order[:4]] * 130
    if k == 5:
        assert got[1] == (130, 0)


def test_nearest_rows_across_the_sampled_tiles_edges(vg, ctx):
    """The nearest rows straddle the edges of the sampled tiles: 8191 | 8192, 8319 | 8320, 127 | 128, 16383 | 16384.  The rows
    outside come from the main GEMM (whose first tile after a sampled one is tile 1, 65, 129), the rows inside from the sample;
    8 inside rows are planted last so that the threshold (the 8th best of the sample) lies beyond all 14 of them: k = 10 is
    answered without a fall-back."""
    outside = [8191, 8320, 128, 16383, 8190, 8321, 129]
    inside = [8192, 8319, 127, 16384, 8193, 8318, 0]
    order = [r for pair in zip(outside, inside) for r in pair] + [16499, 1, 2, 3, 8200, 8300, 16400, 64]
    rows, q = planted(order, 130, 32)
    got, _ = check_planted(vg, ctx, rows, q, 10)
    assert got[0][0][:, :10].tolist() == [order[:10]] * 130
    assert got[1] == (130, 0)


def test_filter_rejects_planted_rows_of_the_sampled_tiles(vg, ctx):
    """search_flat_filtered (one filter per query): every other planted row is rejected, at a per-query phase, together with a
    random third of the rest.  A rejected row is +Inf in the sample and must not come back from it."""
    rng = np.random.default_rng(5)
    order = [8192, 8191, 0, 8319, 8320, 127, 128, 16384, 16383] + [int(r) for r in rng.permutation(INSIDE[4:120])[:40]]
    nq, k = 130, 10
    rows, q = planted(order, nq, 33)
    mask = rng.random((nq, PLANT_N)) > 1.0 / 3.0
    for i in range(nq):
        mask[i, order[i % 2::2]] = False
        mask[i, order[(i + 1) % 2::2]] = True
    seg = o.FlatSegment(rows, PLANT_DIM)
    got, _ = check_planted(vg, ctx, rows, q, k, search=lambda idx: idx.search_flat_filtered(q, k, mask, 0, scan=idx.SCAN_F32),
                           expect=lambda i: seg.search(q[i], k, mask=mask[i]))
    kept = [[r for j, r in enumerate(order) if j % 2 != i % 2][:k] for i in range(nq)]
    assert got[0][0].tolist() == kept


def test_more_than_cap_rows_pass_part_of_them_sampled(vg, ctx):
    """4200 copies of query 0's nearest row outside the sampled tiles and 5 inside one (rows 8192 ..): fewer than 8 in the
    sample, so the threshold lies above their score and all 4205 pass — more than the 4096 keys a query's list holds.  The
    count that flat_sample_append_kernel sets and the main GEMM adds to must show the overflow: query 0 falls back, as under
    the hook, and the answer is the oracle's (the copies with the smallest row ids)."""
    rng = np.random.default_rng(6)
    n, dim, nq, k = 16500, 64, 130, 10
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    near = (q[0] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    free = np.setdiff1d(np.arange(n), np.concatenate([np.arange(0, 128), np.arange(8192, 8320), np.arange(16384, n)]))
    copies = np.concatenate([rng.permutation(free)[:4200], np.arange(8192, 8197)])
    rows[copies] = near
    got, ref = check_planted(vg, ctx, rows, q, k)
    assert got[1][1] >= 1 and got[1] == ref[1]
    assert got[0][0][0].tolist() == sorted(copies.tolist())[:k]
