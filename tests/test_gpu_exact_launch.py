"""The launch seams of k_exact.hip, at tiny dimensions so that size costs nothing; every output against the oracle.

  batch_kernel, bounded_batch_kernel   more rows than 4096 workgroups of 16 take in one pass: the grid-stride loop
  score_candidates_kernel              more candidates than 64 workgroups of 16 take in one pass (nc > 1024); more queries than one grid's
                                       65535 (vg_score_candidates' q0 loop and its three pointer offsets)
  rerank_kernel                        k = 64 | 65: wave 0's register selection / the bitonic sort in LDS; nc around 64 (the selection's
                                       64-wide passes, the sort's smallest pad) and around 128 (the pad to a power of two); nc < k; nc = 0;
                                       INVALID and ids >= n skipped, a candidate listed twice reported twice, equal scores ordered by id
  vg_rerank's limits                   k = 512 | 513; the LDS key buffer: 20352 | 20353 keys as they are (k <= 64), 16384 | 16385 padded to a
                                       power of two (k > 64)"""
import numpy as np
import pytest

from oracle import oracle as o

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
UNSUPPORTED = -5
PAST_ONE_PASS = 4096 * 16 + 16 + 3          # rows: one pass of the batch kernels' largest grid, one more workgroup, a ragged one


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def best(scores, ids, metric, k):
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.uint32)
    order = np.lexsort((ids, -scores if metric else scores))[:k]
    return ids[order], scores[order]


def rerank_want(base, dim, q, cand, metric, k):
    """Segment.Rerank over the candidates that name a row, the k best by (score, id), padded with INVALID and the worst score"""
    cand = np.asarray(cand, np.uint32)
    valid = cand[(cand != INVALID) & (cand < base.shape[0])]
    eid, esc = best(o.rerank_f32(base, dim, q, valid, metric), valid, metric, k) if valid.size else (valid, np.zeros(0, np.float32))
    ids = np.full(k, INVALID, np.uint32)
    sc = np.full(k, -np.inf if metric else np.inf, np.float32)
    ids[:eid.size], sc[:eid.size] = eid, esc
    return ids, sc


# ---- batch and bounded kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 65])
def test_batch_kernels_past_one_pass_of_the_grid(vg, ctx, dim):
    rng = np.random.default_rng(dim)
    n = PAST_ONE_PASS
    q = rng.standard_normal(dim).astype(np.float32)
    t = rng.standard_normal(n * dim).astype(np.float32)
    assert np.array_equal(bits(vg.squared_l2_batch(ctx, q, t, dim)), bits(o.l2_batch(q, t, dim)))
    assert np.array_equal(bits(vg.dot_batch(ctx, q, t, dim)), bits(o.dot_batch(q, t, dim)))


@pytest.mark.parametrize("dim", [4, 65])
def test_bounded_kernel_past_one_pass_of_the_grid(vg, ctx, dim):
    """per-row bounds and one shared bound; a squared distance here is 2 dim +- sqrt(8 dim), so 2 dim splits the rows about evenly"""
    rng = np.random.default_rng(10 + dim)
    n = PAST_ONE_PASS
    q = rng.standard_normal(dim).astype(np.float32)
    t = rng.standard_normal((n, dim)).astype(np.float32)
    per_row = ((1.0 + 2.0 * rng.random(n)) * dim).astype(np.float32)
    shared = np.float32(2.0 * dim)
    d1, e1 = vg.squared_l2_bounded_batch(ctx, q, t.ravel(), dim, per_row)
    d2, e2 = vg.squared_l2_bounded_batch(ctx, q, t.ravel(), dim, shared)
    w1, x1, w2, x2 = np.empty(n, np.float32), np.empty(n, bool), np.empty(n, np.float32), np.empty(n, bool)
    for i in range(n):
        w1[i], x1[i] = o.l2_bounded(q, t[i], float(per_row[i]))
        w2[i], x2[i] = o.l2_bounded(q, t[i], float(shared))
    assert np.array_equal(bits(d1), bits(w1)) and np.array_equal(e1 != 0, x1)
    assert np.array_equal(bits(d2), bits(w2)) and np.array_equal(e2 != 0, x2)
    for x in (x1, x2):                                       # both outcomes, in the first pass of the grid and past it
        assert 0 < x[:65536].sum() < 65536 and 0 < x[65536:].sum() < n - 65536


# ---- score_candidates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
def test_score_candidates_past_one_pass_of_the_grid(vg, ctx, metric):
    rng = np.random.default_rng(20 + metric)
    n, dim, nq, nc = 300, 8, 2, 1024 + 17
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    cand = rng.integers(0, n, (nq, nc)).astype(np.uint32)
    cand[0, 5] = cand[1, 1030] = INVALID                     # skipped: the worst score
    cand[0, 1029] = cand[1, 7] = n + 4                       # an id past the rows: skipped like INVALID
    sc = idx.score_candidates(q, cand)
    worst = np.float32(-np.inf if metric else np.inf)
    for qi in range(nq):
        valid = cand[qi] < n
        assert np.count_nonzero(~valid) == 2
        assert np.array_equal(bits(sc[qi][valid]), bits(o.rerank_f32(base, dim, q[qi], cand[qi][valid], metric))), qi
        assert np.all(bits(sc[qi][~valid]) == bits(worst)), qi
    idx.close()


@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
def test_score_candidates_past_one_grid_of_queries(vg, ctx, metric):
    """65535 + 3 queries drawn from 16 vectors, each vector with its own three candidates: the oracle scores the 16, and every output
    row equals its vector's (a second launch that starts at the wrong query, candidate or output row does not)"""
    rng = np.random.default_rng(30 + metric)
    n, dim, nq, nc, distinct = 200, 4, 65535 + 3, 3, 16
    base = rng.standard_normal((n, dim)).astype(np.float32)
    vecs = rng.standard_normal((distinct, dim)).astype(np.float32)
    vcand = np.stack([rng.permutation(n)[:nc] for _ in range(distinct)]).astype(np.uint32)
    want = np.stack([o.rerank_f32(base, dim, vecs[v], vcand[v], metric) for v in range(distinct)])
    assert np.unique(bits(want)).size == distinct * nc       # (no two of the 48 scores are equal: a row of output names its vector)
    which = rng.integers(0, distinct, nq)
    which[65535:] = [3, 11, 6]                               # the second launch's queries differ from the first launch's first three
    which[:3] = [9, 0, 14]
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    sc = idx.score_candidates(vecs[which], vcand[which])
    assert sc.shape == (nq, nc)
    first = np.array([np.flatnonzero(which == v)[0] for v in range(distinct)])
    assert np.array_equal(bits(sc[first]), bits(want))
    assert np.array_equal(bits(sc), bits(sc[first][which]))
    idx.close()


# ---- rerank -------------------------------------------------------------------------------------------------------------------------
# (k, nc) at a seam: k = 64 | 65 against every nc; the other k where nc meets k, the selection's 64-wide pass or the sort's pad
RERANK_SEAMS = {
    1: (0, 1, 65),
    63: (63, 64, 65),
    64: (0, 1, 63, 64, 65, 100, 128, 129, 700),
    65: (0, 1, 63, 64, 65, 100, 128, 129, 700),
    512: (64, 129, 700),
}

_rerank = {}


def rerank_rows(metric):
    """300 rows of 8 floats, rows 7 and 11 equal (their scores tie: the id decides); Cosine: normalised rows and queries"""
    if metric not in _rerank:
        rng = np.random.default_rng(40 + metric)
        base = rng.standard_normal((300, 8)).astype(np.float32)
        q = rng.standard_normal((3, 8)).astype(np.float32)
        if metric == 1:
            base /= np.linalg.norm(base, axis=1, keepdims=True)
            q /= np.linalg.norm(q, axis=1, keepdims=True)
        base[11] = base[7]
        _rerank[metric] = (base, q)
    return _rerank[metric]


def rerank_lists(rng, n, nq, nc):
    """candidate lists with, where they are long enough to hold them: one INVALID, one id >= n, one candidate listed twice, and the
    two rows that hold equal vectors; the last query's list names no row at all"""
    cand = rng.integers(0, n, (nq, nc)).astype(np.uint32)
    if nc >= 8:
        for qi in range(nq):
            at = rng.permutation(nc)[:6]
            cand[qi, at[0]] = INVALID
            cand[qi, at[1]] = n + qi
            cand[qi, at[2]] = cand[qi, at[3]]
            cand[qi, at[4]], cand[qi, at[5]] = 11, 7
    if nc:
        cand[nq - 1] = np.where(rng.random(nc) < 0.5, INVALID, n + 1).astype(np.uint32)
    return cand


@pytest.mark.parametrize("k", sorted(RERANK_SEAMS))
@pytest.mark.parametrize("metric", [0, 1, 2], ids=["l2", "cosine", "dot"])
def test_rerank_at_its_seams(vg, ctx, metric, k):
    base, q = rerank_rows(metric)
    n, dim = base.shape
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    rng = np.random.default_rng(100 * metric + k)
    for nc in RERANK_SEAMS[k]:
        cand = rerank_lists(rng, n, q.shape[0], nc)
        ids, sc = idx.rerank(q, cand, k)
        assert ids.shape == (q.shape[0], k) and sc.shape == (q.shape[0], k)
        for qi in range(q.shape[0]):
            eid, esc = rerank_want(base, dim, q[qi], cand[qi], metric, k)
            assert np.array_equal(ids[qi], eid), (nc, qi, ids[qi], eid)
            assert np.array_equal(bits(sc[qi]), bits(esc)), (nc, qi)
        if nc >= 8:                                          # what the lists were made to hold is in the answers
            assert np.all(ids[-1] == INVALID)
            if k >= nc:                                      # everything valid is reported: the duplicate twice, 7 before 11
                for qi in range(q.shape[0] - 1):
                    got = ids[qi][ids[qi] != INVALID]
                    assert got.size == nc - 2 and np.unique(got).size < got.size
                    at7, at11 = np.flatnonzero(got == 7), np.flatnonzero(got == 11)
                    assert at11[0] == at7[-1] + 1 and bits(sc[qi][at7[0]]) == bits(sc[qi][at11[0]])
    idx.close()


# ---- limits -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(vg, ctx):
    rng = np.random.default_rng(50)
    base = rng.standard_normal((300, 8)).astype(np.float32)
    idx = vg.Index(ctx, 300, 8)
    idx.set_vectors(base)
    return idx, base, rng.standard_normal((1, 8)).astype(np.float32)


def test_rerank_k_limit(vg, wide):
    idx, base, q = wide
    cand = np.arange(40, dtype=np.uint32)[None, :]
    ids, sc = idx.rerank(q, cand, 512)
    eid, esc = rerank_want(base, 8, q[0], cand[0], 0, 512)
    assert np.array_equal(ids[0], eid) and np.array_equal(bits(sc[0]), bits(esc))
    with pytest.raises(vg.VecgoHipError) as e:
        idx.rerank(q, cand, 513)
    assert e.value.status == UNSUPPORTED and "k=513 exceeds 512" in e.value.message


@pytest.mark.parametrize("k,fits", [(10, 20352), (65, 16384)])
def test_rerank_lds_key_buffer(vg, wide, k, fits):
    """the keys of one query live in LDS: as many as were handed in up to k = 64, padded to a power of two for the sort above"""
    idx, base, q = wide
    rng = np.random.default_rng(fits)
    cand = rng.integers(0, 300, (1, fits + 1)).astype(np.uint32)
    ids, sc = idx.rerank(q, cand[:, :fits], k)
    eid, esc = rerank_want(base, 8, q[0], cand[0, :fits], 0, k)
    assert np.array_equal(ids[0], eid) and np.array_equal(bits(sc[0]), bits(esc))
    with pytest.raises(vg.VecgoHipError) as e:
        idx.rerank(q, cand, k)
    assert e.value.status == UNSUPPORTED and f"nc={fits + 1}" in e.value.message and "LDS key buffer" in e.value.message
