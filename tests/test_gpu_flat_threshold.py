"""Engine.SearchThreshold over one flat segment on the GPU (vg_search_flat_threshold) vs the oracle: flat.Segment.Search(q,
max_results) (flat/segment.go:447-721, the reference's heap, NaN included) followed by the engine's filter (engine.go:1518-1529).
Every case compares ids, score bits and counts; the slots after a query's count hold 0xFFFFFFFF and +Inf (L2) / -Inf (Dot)."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests.test_flat_threshold_cpu import threshold_filter

pytestmark = pytest.mark.gpu

L2, COS, DOT = o.METRIC_L2, o.METRIC_COSINE, o.METRIC_DOT
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same_scores(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def expected(base, dim, q, t, max_results, metric, mask=None):
    if mask is None:
        eid, esc = o.flat_search_f32(base, dim, q, max_results, metric)
    else:
        eid, esc = o.FlatSegment(base, dim, metric).search(q, max_results, mask=mask)
    return threshold_filter(eid, esc, np.float32(t), metric)


def verify(ids, sc, cnt, base, dim, q, thr, max_results, metric, rows, mask=None):
    pad = np.float32(np.inf if metric == L2 else -np.inf)
    for i in rows:
        mi = None if mask is None else (mask if mask.ndim == 1 else mask[i])
        eid, esc = expected(base, dim, q[i], thr[i], max_results, metric, mi)
        c = eid.size
        assert cnt[i] == c, (i, cnt[i], c)
        assert np.array_equal(ids[i, :c], eid), (i, ids[i, :c][:20], eid[:20])
        assert same_scores(sc[i, :c], esc), i
        assert np.all(ids[i, c:] == INVALID) and np.all(bits(sc[i, c:]) == bits(pad)), i


def rank_thresholds(base, dim, q, metric, ranks, exact_rows):
    """one threshold per query at the score of its ranks[i % len]-th row ('none' keeps nothing, 'all' everything): exact
    (the oracle's score) for the queries in exact_rows, from a float64 product for the others"""
    n = base.shape[0]
    none_t, all_t = (np.float32(-1.0), np.float32(np.inf)) if metric == L2 else (np.float32(np.inf), np.float32(-np.inf))
    b64 = base.astype(np.float64)
    thr = np.empty(q.shape[0], np.float32)
    for i in range(q.shape[0]):
        r = ranks[i % len(ranks)]
        if r == "none":
            thr[i] = none_t
        elif r == "all" or r >= n:
            thr[i] = all_t
        elif i in exact_rows:
            _, esc = o.flat_search_f32(base, dim, q[i], r, metric)
            thr[i] = esc[r - 1]
        else:
            s = ((b64 - q[i].astype(np.float64)) ** 2).sum(1) if metric == L2 else b64 @ q[i].astype(np.float64)
            thr[i] = np.partition(s, r - 1)[r - 1] if metric == L2 else -np.partition(-s, r - 1)[r - 1]
    return thr


def checked_rows(nq, most=8):
    return sorted(set(np.linspace(0, nq - 1, min(nq, most)).astype(int).tolist()))


def test_reference_case_on_the_gpu(vg, ctx):
    """internal/engine/batch_test.go:47-67"""
    base = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    idx = vg.Index(ctx, 3, 2)
    idx.set_vectors(base)
    q = np.array([[1, 0], [1, 0]], np.float32)
    ids, sc, cnt = idx.search_flat_threshold(q, [0.5, 1.1], 10)
    assert cnt.tolist() == [1, 2]
    assert ids[0, :1].tolist() == [0] and ids[1, :2].tolist() == [0, 2]
    assert sc[1, :2].tolist() == [0.0, 1.0]
    assert np.all(ids[0, 1:] == INVALID) and np.all(np.isposinf(sc[0, 1:]))


RANKS = ["none", 1, 10, 500, 5000, "all"]


@pytest.mark.parametrize("n,dim,metric,nq,max_results", [
    (40, 30, L2, 3, 10),           # fewer rows than most ranks; dim under one 64-float block (pairs scored from memory)
    (2000, 64, DOT, 9, 100),       # one pass of 8 queries and one of 1
    (5000, 100, COS, 8, 513),      # above vg_search_flat's k limit
    (20000, 128, L2, 64, 4096),
    (30000, 768, DOT, 129, 1),
    (10000, 128, L2, 1024, 10),
    (200000, 768, L2, 1, 16384),   # 'none' only: see the next case
    (200000, 768, DOT, 6, 16384),  # 'all' of 200k rows: a list longer than the LDS buffer (radix select)
])
def test_grid_matches_oracle(vg, ctx, n, dim, metric, nq, max_results):
    rng = np.random.default_rng(n + dim + nq + max_results)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    rows = checked_rows(nq, 6 if n >= 100000 else 8)
    thr = rank_thresholds(base, dim, q, metric, RANKS, set(rows))
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    ids, sc, cnt = idx.search_flat_threshold(q, thr, max_results)
    verify(ids, sc, cnt, base, dim, q, thr, max_results, metric, rows)


def test_ties_duplicates_and_boundary(vg, ctx):
    """duplicated rows tie on the score: they are kept by row id, and a threshold equal to a score keeps that score"""
    rng = np.random.default_rng(11)
    uniq = np.floor(rng.standard_normal((500, 64)) * 2).astype(np.float32)
    base = np.concatenate([uniq] * 6)[rng.permutation(3000)]
    q = np.floor(rng.standard_normal((9, 64)) * 2).astype(np.float32)
    for metric in (L2, DOT):
        idx = vg.Index(ctx, 3000, 64, vg.Metric(metric))
        idx.set_vectors(base)
        thr = rank_thresholds(base, 64, q, metric, [1, 7, 40, 300, 1000], set(range(9)))
        for max_results in (5, 64, 700):
            ids, sc, cnt = idx.search_flat_threshold(q, thr, max_results)
            verify(ids, sc, cnt, base, 64, q, thr, max_results, metric, range(9))


def test_infinite_and_nan_thresholds(vg, ctx):
    rng = np.random.default_rng(12)
    base = rng.standard_normal((3000, 128)).astype(np.float32)
    q = rng.standard_normal((5, 128)).astype(np.float32)
    for metric in (L2, DOT):
        idx = vg.Index(ctx, 3000, 128, vg.Metric(metric))
        idx.set_vectors(base)
        thr = np.array([np.inf, -np.inf, np.nan, np.inf, -np.inf], np.float32)
        ids, sc, cnt = idx.search_flat_threshold(q, thr, 600)
        verify(ids, sc, cnt, base, 128, q, thr, 600, metric, range(5))
        assert cnt[2] == 0
        everything = 0 if metric == L2 else 1
        assert cnt[everything] == 600 and cnt[1 - everything] == 0


@pytest.mark.parametrize("metric", [L2, COS])
@pytest.mark.parametrize("nq,k", [(1, 10), (3, 64), (9, 512), (130, 100)])
def test_no_threshold_equals_search_flat(vg, ctx, metric, nq, k):
    """+Inf (L2) / -Inf (Dot, Cosine) keeps every row: the answer is vg_search_flat(k = max_results), bit for bit"""
    rng = np.random.default_rng(nq + k)
    base = rng.standard_normal((20000, 768)).astype(np.float32)
    q = rng.standard_normal((nq, 768)).astype(np.float32)
    idx = vg.Index(ctx, 20000, 768, vg.Metric(metric))
    idx.set_vectors(base)
    fid, fsc = idx.search_flat(q, k)
    ids, sc, cnt = idx.search_flat_threshold(q, np.inf if metric == L2 else -np.inf, k)
    assert np.all(cnt == k)
    assert np.array_equal(ids, fid) and np.array_equal(bits(sc), bits(fsc))


@pytest.mark.parametrize("metric", [L2, DOT])
def test_masks(vg, ctx, metric):
    rng = np.random.default_rng(13 + metric)
    n, dim, nq = 6000, 128, 10
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    thr = rank_thresholds(base, dim, q, metric, [5, 200, 2000, "all"], set(range(nq)))
    per_query = rng.random((nq, n)) < 0.3
    shared = rng.random(n) < 0.05
    for mask in (per_query, shared):
        ids, sc, cnt = idx.search_flat_threshold(q, thr, 700, mask=mask)
        verify(ids, sc, cnt, base, dim, q, thr, 700, metric, range(nq), mask=mask)


def test_bf16_filter_leaves_the_answer_unchanged(vg, ctx):
    rng = np.random.default_rng(14)
    base = rng.standard_normal((30000, 768)).astype(np.float32)
    q = rng.standard_normal((70, 768)).astype(np.float32)
    idx = vg.Index(ctx, 30000, 768, vg.Metric.DOT)
    idx.set_vectors(base)
    thr = rank_thresholds(base, 768, q, DOT, [3, 100, 2000], {0, 35, 69})
    a = idx.search_flat_threshold(q, thr, 1000)
    idx.enable_bf16_filter(True)
    b = idx.search_flat_threshold(q, thr, 1000)   # 70 queries: nominated on the bf16 rows
    idx.enable_bf16_filter(False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    verify(*a, base, 768, q, thr, 1000, DOT, [0, 35, 69])


@pytest.mark.parametrize("metric", [L2, DOT])
def test_nan_and_inf_scores(vg, ctx, metric):
    """a NaN query, Inf rows, dot products that overflow to +Inf and to -Inf: the reference's heap (replayed) decides what
    Search returns, the filter what is kept"""
    rng = np.random.default_rng(15 + metric)
    n, dim = 3000, 64
    base = rng.standard_normal((n, dim)).astype(np.float32)
    base[17, 3] = np.inf
    base[900, 0] = -np.inf
    base[1200] = 3e19
    base[1201] = -3e19
    q = rng.standard_normal((6, dim)).astype(np.float32)
    q[1, 5] = np.nan
    q[2] = 3e19
    q[3] = -3e19
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    big = np.float32(np.inf if metric == L2 else -np.inf)
    for thr in (np.full(6, big), np.array([0.0, 5.0, 1e30, -1e30, 100.0, big], np.float32)):
        # 6 queries: the scan; 12: the nomination (the bound is not finite: every proof fails and the scan answers);
        # 16384: the heap replay holds more than 64 KiB of LDS
        for qq, tt in ((q, thr), (np.concatenate([q, q]), np.concatenate([thr, thr]))):
            for max_results in (10, 600, 16384):
                ids, sc, cnt = idx.search_flat_threshold(qq, tt, max_results)
                verify(ids, sc, cnt, base, dim, qq, tt, max_results, metric, range(qq.shape[0]))


@pytest.mark.parametrize("hook", ["VG_FLAT_FORCE_EXACT", "VG_FLAT_NO_SCAN", "VG_NO_CAND_REPLAY"])
def test_hooks_give_the_same_answer(vg, ctx, hook):
    rng = np.random.default_rng(16)
    n, dim, nq = 20000, 256, 12
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric.L2)
    idx.set_vectors(base)
    thr = rank_thresholds(base, dim, q, L2, RANKS, set(range(nq)))
    s_ = idx.flat_stats()
    a = idx.search_flat_threshold(q, thr, 2000)   # 12 queries: the nomination; random rows: the proofs hold
    s0 = idx.flat_stats()
    assert s0[0] - s_[0] == nq and s0[1] - s_[1] <= 1
    hooks.set_hook(hook, 1)
    try:
        b = idx.search_flat_threshold(q, thr, 2000)
    finally:
        hooks.set_hook(hook, 0)
    s1 = idx.flat_stats()
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    verify(*a, base, dim, q, thr, 2000, L2, range(nq))
    assert s1[0] - s0[0] == nq
    if hook == "VG_FLAT_FORCE_EXACT":
        assert s1[1] - s0[1] == nq
    else:
        assert s1[1] - s0[1] <= 1


def test_poor_sample_falls_back_to_the_scan(vg, ctx):
    """Rows sorted farthest first from the queries: every sampled tile is far, the sample threshold lets far more rows through
    than a list holds, every query's list overflows and its proof fails; the scan answers them, exactly."""
    rng = np.random.default_rng(17)
    n, dim, nq = 40000, 64, 12
    base = rng.standard_normal((n, dim)).astype(np.float32)
    centre = rng.standard_normal(dim).astype(np.float32)
    base = np.ascontiguousarray(base[np.argsort(-((base - centre) ** 2).sum(1))])
    q = (centre + rng.standard_normal((nq, dim)).astype(np.float32) * 0.01).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric.L2)
    idx.set_vectors(base)
    s0 = idx.flat_stats()
    thr = np.full(nq, np.inf, np.float32)
    thr[::3] = rank_thresholds(base, dim, q[::3], L2, [3000], set(range(4)))
    ids, sc, cnt = idx.search_flat_threshold(q, thr, 100)
    s1 = idx.flat_stats()
    assert s1[0] - s0[0] == nq and s1[1] - s0[1] > 0
    verify(ids, sc, cnt, base, dim, q, thr, 100, L2, range(nq))


@pytest.mark.parametrize("dim", [64, 100])   # the rows in registers; pairs scored from memory
def test_scattered_fall_back_scans_each_slots_own_query(vg, ctx, dim):
    """The input of test_poor_sample_falls_back_to_the_scan, 17 queries: those with i % 3 == 0 ask for nothing (threshold -1: the
    user's threshold stands, the list is empty, the proof holds), the other 11 for everything (their lists overflow).  The scan
    then answers 11 queries at slots that are not their query numbers, in passes of 8 and 3: slot s reads the query, threshold
    and filter of query qmap[s].  The per-query filter has a different row for every query.
    Rows sorted farthest first leave only the ~7000 rows after the last sampled tile under the sample threshold, and a filter
    that keeps 30 % of them does not overflow a 4096-key list (measured: no fall-back).  So the farthest rows fill the tiles
    the sample reads (every 64th tile of 128 rows) and the rest follow farthest first: every other row passes the sample
    threshold, 30 % of them too."""
    rng = np.random.default_rng(23 + dim)
    n, nq = 40000, 17
    base = rng.standard_normal((n, dim)).astype(np.float32)
    centre = rng.standard_normal(dim).astype(np.float32)
    far_first = np.argsort(-((base - centre) ** 2).sum(1))
    sampled = (np.arange(n) // 128) % 64 == 0
    order = np.empty(n, np.int64)
    order[sampled] = far_first[:sampled.sum()]
    order[~sampled] = far_first[sampled.sum():]
    base = np.ascontiguousarray(base[order])
    q = (centre + rng.standard_normal((nq, dim)).astype(np.float32) * 0.01).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric.L2)
    idx.set_vectors(base)
    thr = np.full(nq, np.inf, np.float32)
    thr[::3] = -1.0
    per_query = rng.random((nq, n)) < 0.3
    for mask in (None, per_query):
        s0 = idx.flat_stats()
        ids, sc, cnt = idx.search_flat_threshold(q, thr, 100, mask=mask)
        s1 = idx.flat_stats()
        assert s1[0] - s0[0] == nq and s1[1] - s0[1] == 11, (s1[0] - s0[0], s1[1] - s0[1])
        verify(ids, sc, cnt, base, dim, q, thr, 100, L2, range(nq), mask=mask)


def test_clustered_corpus(vg, ctx):
    """rows in tight clusters around a few centres (thousands of near-equal scores around every threshold); a batch is
    nominated, and what its proofs leave is scanned"""
    rng = np.random.default_rng(17)
    n, dim, nq = 40000, 128, 16
    centres = rng.standard_normal((8, dim)).astype(np.float32) * 10
    base = (centres[rng.integers(0, 8, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.01).astype(np.float32)
    q = (centres[rng.integers(0, 8, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.01).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric.L2)
    idx.set_vectors(base)
    s0 = idx.flat_stats()
    thr = rank_thresholds(base, dim, q, L2, [10, 3000, 9000, "all"], set(range(nq)))
    for max_results in (100, 16384):
        ids, sc, cnt = idx.search_flat_threshold(q, thr, max_results)
        verify(ids, sc, cnt, base, dim, q, thr, max_results, L2, range(nq))
    s1 = idx.flat_stats()
    assert s1[0] - s0[0] == 2 * nq and s1[1] - s0[1] > 0


def test_small_batch_through_the_nomination(vg, ctx):
    """VG_FLAT_NO_SCAN: a batch of up to 8 queries is nominated too; same answer as the scan"""
    rng = np.random.default_rng(21)
    n, dim, nq = 30000, 100, 5
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    for metric in (L2, DOT):
        idx = vg.Index(ctx, n, dim, vg.Metric(metric))
        idx.set_vectors(base)
        thr = rank_thresholds(base, dim, q, metric, ["none", 3, 700, 9000, "all"], set(range(nq)))
        a = idx.search_flat_threshold(q, thr, 5000)
        hooks.set_hook("VG_FLAT_NO_SCAN", 1)
        try:
            b = idx.search_flat_threshold(q, thr, 5000)
        finally:
            hooks.set_hook("VG_FLAT_NO_SCAN", 0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
        verify(*b, base, dim, q, thr, 5000, metric, range(nq))


def test_limits(vg, ctx):
    rng = np.random.default_rng(18)
    base = rng.standard_normal((500, 32)).astype(np.float32)
    q = rng.standard_normal((2, 32)).astype(np.float32)
    idx = vg.Index(ctx, 500, 32)
    idx.set_vectors(base)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_flat_threshold(q, 1.0, 16385)
    assert e.value.status == -5 and "16385" in e.value.message
    ids, sc, cnt = idx.search_flat_threshold(q, 1e9, 16384)   # the largest max_results: every row kept
    assert cnt.tolist() == [500, 500]
    # nothing to search: no-ops that write nothing
    out = (np.full((0, 5), 7, np.uint32), np.zeros((0, 5), np.float32), np.zeros(0, np.int32))
    idx.search_flat_threshold(np.zeros((0, 32), np.float32), [], 5, out=out)
    ids, sc, cnt = idx.search_flat_threshold(q, 1.0, 0)
    assert ids.shape == (2, 0)
    # a partitioned segment: the reference would probe some partitions only
    pidx = vg.Index(ctx, 500, 32)
    pidx.set_vectors(base)
    pidx.set_partitions(base[:4].copy(), np.array([0, 100, 200, 300, 500], np.uint32))
    with pytest.raises(vg.VecgoHipError) as e:
        pidx.search_flat_threshold(q, 1.0, 10)
    assert e.value.status == -5
    hidx = vg.Index(ctx, 500, 32, vg.Metric.HAMMING)
    with pytest.raises(vg.VecgoHipError) as e:
        hidx.search_flat_threshold(q, 1.0, 10)
    assert e.value.status == -5


def test_full_size(vg, ctx):
    """1M x 768, 1024 queries: thresholds at rank 100 (max_results 1000) and rank 5000 (max_results 16384)"""
    import torch
    rng = np.random.default_rng(19)
    n, dim, nq = 1_000_000, 768, 1024
    base = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((nq, dim), dtype=np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric.L2)
    idx.set_vectors(base)
    rows = checked_rows(nq, 16)
    # rank 100: vg_search_flat's 100th score is the threshold (bit-exact with the oracle: tests/test_gpu_flat.py)
    fid, fsc = idx.search_flat(q, 100)
    thr = fsc[:, 99].copy()
    ids, sc, cnt = idx.search_flat_threshold(q, thr, 1000)
    assert np.all(cnt >= 100) and np.array_equal(ids[:, :100], fid) and np.array_equal(bits(sc[:, :100]), bits(fsc))
    for i in range(nq):  # ties with the 100th score are kept after it
        assert np.all(bits(sc[i, 100:cnt[i]]) == bits(thr[i])), i
    verify(ids, sc, cnt, base, dim, q, thr, 1000, L2, rows)
    # rank 5000: float64 thresholds (exact, the oracle's score, for the checked queries); every count against a float64 count of
    # the rows within, up to rounding
    dev = torch.device("cuda")
    tb = torch.from_numpy(base).to(dev, torch.float64)
    bn = (tb * tb).sum(1)

    def scores64(q0):
        tq = torch.from_numpy(q[q0:q0 + 64]).to(dev, torch.float64)
        return bn[None, :] - 2 * tq @ tb.T + (tq * tq).sum(1)[:, None]

    thr = np.concatenate([scores64(q0).kthvalue(5000, dim=1).values.float().cpu().numpy() for q0 in range(0, nq, 64)])
    for i in rows:
        thr[i] = o.flat_search_f32(base, dim, q[i], 5000, L2)[1][4999]
    ids, sc, cnt = idx.search_flat_threshold(q, thr, 16384)
    verify(ids, sc, cnt, base, dim, q, thr, 16384, L2, rows)
    for q0 in range(0, nq, 64):
        s = scores64(q0)
        t = torch.from_numpy(thr[q0:q0 + 64]).to(dev, torch.float64)[:, None]
        eps = 1e-4 * t.abs() + 1e-3
        lo = (s < t - eps).sum(1).clamp(max=16384).cpu().numpy()
        hi = (s <= t + eps).sum(1).clamp(max=16384).cpu().numpy()
        c = cnt[q0:q0 + 64]
        assert np.all((lo <= c) & (c <= hi)), q0
        assert np.all((c >= 4900) & (c <= 5100)), q0
