"""The search walks' split of a batch over several launches (WalkChunks, vg_search.hpp).  A launch takes as many queries as
scratch_cap holds scratch for — on this card every test batch —, yet each walker offsets its operands per launch: queries,
masks (a shared mask has stride 0), outputs, stats and counts batch-relative by q0, the PQ tables, RaBitQ query codes, `redo`
marks, HBM heaps and visited bitmaps launch-relative or batch-relative as each is laid out.  Under the test hook
VG_WALK_SMALL_SCRATCH a launch takes at most 5 queries, so 13 queries walk in launches of 5, 5 and 3.  Every entry point with
the hook on must answer what it answers with it off, bit for bit — ids, scores, stats, counts —, and the first and last query
of each launch must equal the oracle."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import vamana_fresh_ref as fresh
from tests.hooks import set_hook
from tests.test_gpu_graph import bits
from tests.test_gpu_hnsw_scorers import case as hnsw_case, compare as hnsw_compare
from tests.test_gpu_vamana_large_k import same_scores
from tests.test_gpu_vamana_scorers import KIND, case as vamana_case
from tests.threshold_ref import engine_filter

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
N, NQ, CHUNK = 700, 13, 5          # the cases' rows (both scorer modules build 700); the hook's queries per launch
EDGES = (0, 4, 5, 9, 10, 12)       # the first and last query of each launch
assert [min(CHUNK, NQ - q0) for q0 in range(0, NQ, CHUNK)] == [5, 5, 3]
assert sorted(EDGES) == sorted({q for q0 in range(0, NQ, CHUNK) for q in (q0, min(q0 + CHUNK, NQ) - 1)})


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def queries(dim, seed):
    return np.random.default_rng(seed).standard_normal((NQ, dim)).astype(np.float32)


def whole_and_split(call):
    """call() with the hook off, then on: the two answers equal bit for bit; returns the split one"""
    whole = call()
    set_hook("VG_WALK_SMALL_SCRATCH", 1)
    try:
        split = call()
    finally:
        set_hook("VG_WALK_SMALL_SCRATCH", 0)
    assert len(whole) == len(split)
    for i, (a, b) in enumerate(zip(whole, split)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, i
        raw = [np.ascontiguousarray(x).reshape(NQ, -1).view(np.uint8) for x in (a, b)]   # bytes: a NaN equals itself only bit for bit
        differ = np.nonzero((raw[0] != raw[1]).any(1))[0]
        assert differ.size == 0, (f"output {i}: queries {differ.tolist()} differ between one launch and launches of {CHUNK}",
                                  a[differ[0]], b[differ[0]])
    return split


# ---- the HNSW walks (search_hnsw_impl, vg_search_hnsw_predicate) ------------------------------------------------------------------
@pytest.mark.parametrize("ef", [64, 600])    # LDS heaps; split heaps: heap_ws per launch
def test_hnsw_f32(vg, ctx, ef):
    idx, oidx, search, _, _ = hnsw_case(vg, ctx, "f32", 100, 0)
    q = queries(100, 1)
    q[7, 33] = np.inf                        # in the second launch: its `redo` mark is the launch's third
    assert oidx.search(q[7], 10, ef)[2].pops >= 1
    got = whole_and_split(lambda: search(q, 10, ef, stats=True))
    hnsw_compare(got, lambda qi: oidx.search(q[qi], 10, ef), EDGES + (7,))


@pytest.mark.parametrize("ef", [64, 600])
@pytest.mark.parametrize("dim,m", [(64, 16), (128, 16)], ids=["table", "direct"])   # table: `luts` rebuilt per launch
def test_hnsw_pq(vg, ctx, dim, m, ef):
    idx, oidx, search, _, _ = hnsw_case(vg, ctx, "pq", dim, m)
    q = queries(dim, 2)
    q[7, dim // 3] = np.inf
    got = whole_and_split(lambda: search(q, 10, ef, stats=True))
    hnsw_compare(got, lambda qi: oidx.search(q[qi], 10, ef), EDGES + (7,))


@pytest.mark.parametrize("per_query", [False, True], ids=["shared", "per_query"])   # shared: stride 0
def test_hnsw_filtered(vg, ctx, per_query):
    idx, oidx, _, _, _ = hnsw_case(vg, ctx, "f32", 100, 0)
    q = queries(100, 3)
    mask = np.random.default_rng(4).random((NQ, N) if per_query else N) < 0.6
    got = whole_and_split(lambda: idx.search_hnsw_filtered(q, 10, 64, mask, 0.6, stats=True))
    hnsw_compare(got, lambda qi: oidx.search_filtered(q[qi], 10, 64, mask[qi] if per_query else mask, 0.6), EDGES)


def test_hnsw_predicate(vg, ctx):
    idx, oidx, _, _, _ = hnsw_case(vg, ctx, "f32", 100, 0)
    q = queries(100, 5)
    sel = np.random.default_rng(6).random((NQ, N)) < 0.2
    got = whole_and_split(lambda: idx.search_hnsw_predicate(q, 10, 64, sel, stats=True))
    hnsw_compare(got, lambda qi: oidx.search_predicate(q[qi], 10, 64, sel[qi]), EDGES)


# ---- the Vamana walks (vamana_impl) ----------------------------------------------------------------------------------------------
def vamana_compare(got, want, metric=0):
    ids, sc, st = got
    pad = np.float32(-np.inf if metric != 0 else np.inf)
    for qi in EDGES:
        eid, esc, est = want(qi)
        r = eid.size
        assert np.array_equal(ids[qi, :r], eid), (qi, ids[qi], eid)
        assert same_scores(sc[qi, :r], esc), qi
        assert np.all(ids[qi, r:] == INVALID) and np.all(bits(sc[qi, r:]) == bits(pad)), (qi, r)
        assert (int(st[qi][0]), int(st[qi][1]), int(st[qi][3])) == (est.nodes_visited, est.distance_computations, est.pops), qi


# PQ as table (`luts + q0 * pq_m * 256`) and direct; INT4 from the table and in place; RaBitQ (`qcodes + q0 * (rq_nb + 4)`)
VAMANA = [("f32", 100, 0), ("pq", 64, 16), ("pq", 128, 16), ("int4", 47, 0), ("int4", 32, 0), ("rabitq", 576, 0)]


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("scorer,dim,arg", VAMANA)
def test_vamana(vg, ctx, scorer, dim, arg, k):
    idx, ov, _, _, metric = vamana_case(vg, ctx, scorer, dim, arg)
    q = queries(dim, 7)
    got = whole_and_split(lambda: idx.search_vamana(q, k, kind=KIND[scorer], stats=True))
    vamana_compare(got, lambda qi: ov.search(q[qi], k), metric)


@pytest.mark.parametrize("scorer,dim,arg", [("pq", 64, 16), ("rabitq", 576, 0)])
def test_vamana_filtered(vg, ctx, scorer, dim, arg):
    idx, ov, _, _, metric = vamana_case(vg, ctx, scorer, dim, arg)
    q = queries(dim, 8)
    masks = np.random.default_rng(9).random((NQ, N)) < 0.3
    got = whole_and_split(lambda: idx.search_vamana_filtered(q, 10, masks, kind=KIND[scorer], stats=True))
    vamana_compare(got, lambda qi: ov.search(q[qi], 10, mask=masks[qi]), metric)


def test_vamana_threshold(vg, ctx):
    idx, ov, _, _, metric = vamana_case(vg, ctx, "f32", 100, 0)
    q = queries(100, 10)
    k = 100
    sc = idx.search_vamana(q, k, kind=0)[1]
    thr = np.ascontiguousarray(sc[np.arange(NQ), 5 + 7 * np.arange(NQ)])    # a count of its own per query: 6, 13, ... (ties aside)
    ids, sc, cnt, st = whole_and_split(lambda: idx.search_vamana_threshold(q, thr, k, kind=0, stats=True))
    assert np.unique(cnt).size > NQ // 2
    for qi in EDGES:
        eid, esc, est = ov.search(q[qi], k)
        e_ids, e_sc, e_cnt = engine_filter(eid, esc, thr[qi], metric != 0, k)
        assert int(cnt[qi]) == e_cnt, (qi, thr[qi])
        assert np.array_equal(ids[qi], e_ids) and same_scores(sc[qi], e_sc), qi
        assert (int(st[qi][0]), int(st[qi][1]), int(st[qi][3])) == (est.nodes_visited, est.distance_computations, est.pops), qi


# ---- vg_search_vamana_fresh ------------------------------------------------------------------------------------------------------
def test_vamana_fresh(vg, ctx):
    rng = np.random.default_rng(11)
    dim = 32
    base = rng.standard_normal((N, dim)).astype(np.float32)
    idx = vg.Index(ctx, 0, dim, vg.Metric(0))
    idx.insert_vamana(base[:400], r=16, l=40, max_batch=64, growth_div=8)
    idx.insert_vamana(base[400:], r=16, l=40, max_batch=64, growth_div=8)
    g, entry = idx.get_vamana_graph()
    q = queries(dim, 12)
    deleted = rng.random(N) < 0.2
    masks = rng.random((NQ, N)) < 0.3
    ids, sc, cnt = whole_and_split(lambda: idx.search_vamana_fresh(q, 10, l=50, deleted=deleted, mask=masks))
    eids, esc, ecnt = fresh.search(base, fresh.lists_of(g), entry, q[list(EDGES)], 10, l=50, deleted=deleted, mask=masks[list(EDGES)])
    assert np.array_equal(cnt[list(EDGES)], ecnt)
    assert np.array_equal(ids[list(EDGES)], eids) and np.array_equal(bits(sc[list(EDGES)]), bits(esc))
    assert not deleted[ids[ids != INVALID]].any()
    idx.close()
