"""The host loops of the flat searches at a second chunk: vg_search_flat walks a batch in chunks of 4096 queries, and every
chunk offsets its queries (q + q0 * dim), its filters (mask + q0 * mask_stride), its results (ids + q0 * k), its proof flags and
work list and the fall-back's patches.  4096 + 130 queries over 4200 rows (33 row tiles, the last ragged; above the 4096-key
list, so the thresholds come from the row sample): the second chunk is a ragged two-tile chunk that still takes the split tile.
Every 37th query against the oracle, every query against the same batch searched as two calls cut at query 2113 (no tile
multiple), ids and score bits."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests.test_gpu_flat_threshold import RANKS, checked_rows, rank_thresholds, verify

pytestmark = pytest.mark.gpu

N, DIM, NQ, CUT = 4200, 32, 4096 + 130, 2113
L2, DOT = o.METRIC_L2, o.METRIC_DOT
CHECKED = range(0, NQ, 37)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


class Data:
    """the rows, the queries, a 30 % filter per query, and the oracle's answers (computed once per (metric, k, filtered))"""

    def __init__(self):
        rng = np.random.default_rng(4226)
        self.base = rng.standard_normal((N, DIM)).astype(np.float32)
        self.q = rng.standard_normal((NQ, DIM)).astype(np.float32)
        self.mask = rng.random((NQ, N)) < 0.3
        self.mask.setflags(write=False)
        self.base.setflags(write=False)
        self.q.setflags(write=False)
        self._exp = {}

    def expected(self, metric, k, filtered):
        key = (metric, k, filtered)
        if key not in self._exp:
            seg = o.FlatSegment(self.base, DIM, metric=metric)
            self._exp[key] = [seg.search(self.q[i], k, 0, mask=self.mask[i]) if filtered else
                              o.flat_search_f32(self.base, DIM, self.q[i], k, metric) for i in CHECKED]
        return self._exp[key]


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def indexes(vg, ctx, data):
    out = {}
    for metric in (L2, DOT):
        out[metric] = vg.Index(ctx, N, DIM, vg.Metric(metric))
        out[metric].set_vectors(data.base)
    return out


def against_oracle(ids, sc, exp):
    for i, (eid, esc) in zip(CHECKED, exp):
        r = eid.size
        assert np.array_equal(ids[i, :r], eid), (i, ids[i, :r][:8], eid[:8])
        assert np.array_equal(bits(sc[i, :r]), bits(esc)), i
        assert np.all(ids[i, r:] == 0xFFFFFFFF), i


def against_two_calls(search, q, ids, sc):
    a, b = search(q[:CUT], slice(0, CUT)), search(q[CUT:], slice(CUT, NQ))
    assert np.array_equal(np.vstack([a[0], b[0]]), ids)
    assert np.array_equal(bits(np.vstack([a[1], b[1]])), bits(sc))


def plain(idx, k):
    return lambda q, rows: idx.search_flat(q, k)


def filtered(idx, k, mask):
    return lambda q, rows: idx.search_flat_filtered(q, k, mask[rows], 0)


@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("k", [5, 40, 60, 100])   # the screen; the split tile, pick + verify; verify-all; verify-sort, a deeper sample
def test_chunks_match_oracle_and_a_cut_batch(data, indexes, metric, k):
    idx = indexes[metric]
    s0 = idx.flat_stats()[0]
    ids, sc = idx.search_flat(data.q, k)
    assert idx.flat_stats()[0] - s0 == NQ
    against_oracle(ids, sc, data.expected(metric, k, False))
    against_two_calls(plain(idx, k), data.q, ids, sc)
    assert idx.flat_stats()[0] - s0 == 2 * NQ


@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("k", [10, 60, 150])
def test_chunks_with_a_filter_per_query(data, indexes, metric, k):
    idx = indexes[metric]
    ids, sc = idx.search_flat_filtered(data.q, k, data.mask, 0)
    against_oracle(ids, sc, data.expected(metric, k, True))
    against_two_calls(filtered(idx, k, data.mask), data.q, ids, sc)


@pytest.mark.parametrize("metric", [L2, DOT])
def test_chunks_under_the_bf16_filter(vg, ctx, data, metric):
    idx = vg.Index(ctx, N, DIM, vg.Metric(metric))
    idx.set_vectors(data.base)
    idx.enable_bf16_filter(True)
    ids, sc = idx.search_flat(data.q, 10)
    against_oracle(ids, sc, data.expected(metric, 10, False))
    against_two_calls(plain(idx, 10), data.q, ids, sc)
    ids, sc = idx.search_flat_filtered(data.q, 10, data.mask, 0)
    against_oracle(ids, sc, data.expected(metric, 10, True))
    against_two_calls(filtered(idx, 10, data.mask), data.q, ids, sc)


# queries answered by the exhaustive kernel in test_fall_back_at_a_chunk_offset, at k = 10 and at k = 100: the counts of the
# commit that added this test (the five planted queries and the random ones whose proof the cluster's norm widens too far)
FALL_BACKS = {10: 5, 100: 5}


def test_fall_back_at_a_chunk_offset(vg, ctx, data):
    """80 rows inside a ball of radius 1e-4 around a centre of norm ~50, five queries at that centre in the second chunk
    (positions 4100 .. 4220): the GEMM-form scores cannot separate the cluster's rows, the five proofs fail, and the exhaustive
    kernel answers them — through the work list, flat_patch (k = 10) and the paged flat_page_patch (k = 100) of a chunk that
    starts at query 4096.  The cluster lies in the sampled row tile (rows 0 .. 127), so that at k = 100 too the five queries'
    thresholds fall inside it and their proofs fail."""
    rng = np.random.default_rng(4)
    centre = rng.standard_normal(DIM).astype(np.float32)
    centre *= np.float32(50.0 / np.linalg.norm(centre))
    base = data.base.copy()
    off = rng.standard_normal((80, DIM))
    off *= 1e-4 * rng.random((80, 1)) / np.linalg.norm(off, axis=1, keepdims=True)
    base[20:100] = (centre + off).astype(np.float32)
    q = data.q.copy()
    planted = [4100, 4130, 4160, 4190, 4220]
    q[planted] = centre
    idx = vg.Index(ctx, N, DIM)
    idx.set_vectors(base)
    fell = {}
    for k in (10, 100):
        s0 = idx.flat_stats()
        ids, sc = idx.search_flat(q, k)
        s1 = idx.flat_stats()
        fell[k] = s1[1] - s0[1]
        print(f"fall-backs at k = {k}: {fell[k]} of {NQ}")
        for i in planted + [0, 37, 4095, 4096, 4097, NQ - 1]:
            eid, esc = o.flat_search_f32(base, DIM, q[i], k)
            assert np.array_equal(ids[i], eid), (k, i, ids[i][:8], eid[:8])
            assert np.array_equal(bits(sc[i]), bits(esc)), (k, i)
        assert s1[0] - s0[0] == NQ
        assert 5 <= fell[k] < NQ // 10
    assert fell == FALL_BACKS


@pytest.mark.parametrize("k", [10, 100])
def test_chunks_force_exact(vg, ctx, data, k):
    idx = vg.Index(ctx, N, DIM)
    idx.set_vectors(data.base)
    hooks.set_hook("VG_FLAT_FORCE_EXACT", 1)
    try:
        ids, sc = idx.search_flat(data.q, k)
    finally:
        hooks.set_hook("VG_FLAT_FORCE_EXACT", 0)
    against_oracle(ids, sc, data.expected(L2, k, False))
    assert idx.flat_stats() == (NQ, NQ)


def test_chunks_unfused(data, indexes):
    idx = indexes[L2]
    hooks.set_hook("VG_FLAT_UNFUSED", 1)
    try:
        ids, sc = idx.search_flat(data.q, 10)
        against_two_calls(plain(idx, 10), data.q, ids, sc)
    finally:
        hooks.set_hook("VG_FLAT_UNFUSED", 0)
    against_oracle(ids, sc, data.expected(L2, 10, False))


@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("nq,max_results", [(130, 16384), (512 + 130, 16384), (NQ, 1000)])
def test_threshold_search_chunks(data, indexes, metric, nq, max_results):
    """vg_search_flat_threshold at max_results = 16384: a query's list holds 65536 keys (more than the rows: no sample) and a
    chunk 512 queries.  130 queries are one chunk, 642 a whole one and a ragged one.  At max_results = 1000 a list holds 4096
    keys, fewer than the rows, so the thresholds come from the row sample, and a chunk 4096 queries: 4226 are a whole chunk and a
    ragged one through the sample.  Each against the oracle on its checked rows (test_grid_matches_oracle's checks) and, every
    query, against the same batch searched as two calls of half the queries."""
    idx = indexes[metric]
    q = data.q[:nq]
    rows = checked_rows(nq)
    thr = rank_thresholds(data.base, DIM, q, metric, RANKS, set(rows))
    ids, sc, cnt = idx.search_flat_threshold(q, thr, max_results)
    verify(ids, sc, cnt, data.base, DIM, q, thr, max_results, metric, rows)
    h = nq // 2
    a, b = idx.search_flat_threshold(q[:h], thr[:h], max_results), idx.search_flat_threshold(q[h:], thr[h:], max_results)
    assert np.array_equal(np.vstack([a[0], b[0]]), ids)
    assert np.array_equal(bits(np.vstack([a[1], b[1]])), bits(sc))
    assert np.array_equal(np.concatenate([a[2], b[2]]), cnt)
