"""diskann.Segment.Search with 512 < k <= 16384 (diskann/segment.go:503-706) and Engine.SearchThreshold's DiskANN leg
(engine/engine.go:1485-1531) on the GPU against the oracle's walk, which takes any k: ids, score bits, order, padding and the
nodes_visited / distance_computations / pops counters, for every node scorer (fp32, PQ, RaBitQ, INT4), every metric, with and
without a row filter."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import graphs
from tests.hooks import set_hook
from tests.test_gpu_graph import bits
from tests.threshold_ref import engine_filter

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF


def same_scores(a, b):
    """score bits equal, any NaN equal to any NaN (as tests/test_gpu_nan.py compares: a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def make(vg, ctx, base, g, entry, kind, metric=0, seed=0):
    """(GPU index, oracle walk) over rows `base` and graph `g` with the node scorer `kind`"""
    n, dim = base.shape
    rng = np.random.default_rng(seed)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vamana_graph(g, entry)
    if kind == 0:
        idx.set_vectors(base)
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_F32, metric=metric, base=base)
    elif kind == 1:
        m = dim // 8
        opq = o.ProductQuantizer(dim, m, 256)
        opq.set_codebooks(rng.integers(-128, 128, m * 256 * 8).astype(np.int8), (rng.random(m) * 0.02 + 0.005).astype(np.float32),
                          ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32))
        codes = opq.encode_batch(base)
        pq = vg.ProductQuantizer(ctx, dim, m, 256)
        pq.set_codebooks(opq.codebooks, opq.scales, opq.offsets)
        idx.set_pq_codes(pq, codes)
        idx._keep = pq
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_PQ, metric=metric, pq=opq, codes=codes)
    elif kind == 2:
        codes = o.rabitq_encode_batch(base, dim)
        idx.set_rabitq_codes(codes)
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_RABITQ, metric=metric, codes=codes)
    else:
        ref = o.Int4Quantizer(dim)
        ref.train(base)
        codes = ref.encode_batch(base)
        iq = vg.Int4Quantizer(ctx, dim)
        iq.train(base)
        idx.set_int4_codes(iq, codes)
        idx._keep = iq
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_INT4, metric=metric, codes=codes, int4_table=ref.table)
    return idx, ov


def check(idx, ov, q, k, kind, mask=None, nq_oracle=None, metric=0):
    if mask is None:
        ids, sc, st = idx.search_vamana(q, k, kind=kind, stats=True)
    else:
        ids, sc, st = idx.search_vamana_filtered(q, k, mask, kind=kind, stats=True)
    assert ids.shape == (q.shape[0], k)
    pad = np.float32(-np.inf if metric != 0 else np.inf)
    out = []
    for qi in range(q.shape[0] if nq_oracle is None else nq_oracle):
        mi = None if mask is None else (mask if mask.ndim == 1 else mask[qi])
        eid, esc, est = ov.search(q[qi], k, mask=mi)
        r_ = eid.size
        assert np.array_equal(ids[qi, :r_], eid), (qi, k)
        assert same_scores(sc[qi, :r_], esc), (qi, k)
        assert np.all(ids[qi, r_:] == INVALID) and np.all(bits(sc[qi, r_:]) == bits(pad)), (qi, r_)
        assert (int(st[qi][0]), int(st[qi][1]), int(st[qi][3])) == (est.nodes_visited, est.distance_computations, est.pops), qi
        out.append((eid, esc, est))
    return ids, sc, st, out


_graphs = {}


def gpu_graph(vg, ctx, base, r, seed=1):
    """a Vamana graph built on the GPU (construction is not under test: the oracle walks the same graph)"""
    n, dim = base.shape
    key = (base.tobytes().__hash__(), r, seed)
    if key in _graphs:
        return _graphs[key]
    b = vg.Index(ctx, n, dim)
    b.set_vectors(base)
    b.build_vamana(r=r, l=max(2 * r, 48), seed=seed)
    g, entry = b.get_vamana_graph()
    b.close()
    _graphs[key] = (g, entry)
    return g, entry


def rows(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


# ---- the grid: kinds x metrics x k, graphs from tests/graphs.py (n <= 8k) ----------------------------------------------------
# (Cosine: the fp32 scorer only — the code scorers answer L2-type distances whatever the metric)
@pytest.mark.parametrize("kind,metric", [(0, 0), (0, 2), (0, 1), (1, 0), (1, 2), (2, 0), (2, 2), (3, 0), (3, 2)])
@pytest.mark.parametrize("n,dim,r,k", [(2000, 16, 16, 513), (3000, 128, 32, 1000), (8000, 16, 16, 4096)])
def test_large_k_matches_oracle(vg, ctx, kind, metric, n, dim, r, k):
    base = rows(n, dim, n + dim + kind)
    if metric == 1:
        base /= np.linalg.norm(base, axis=1, keepdims=True)
    g, entry = graphs.build_vamana(base, r=r, seed=n)
    idx, ov = make(vg, ctx, base, g, entry, kind, metric, seed=kind)
    q = rows(6, dim, 7 + k)
    if metric == 1:
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    check(idx, ov, q, k, kind, metric=metric)
    idx.close()


# ---- larger graphs built on the GPU, k = 16384, dim 768 ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("n,dim,r,k", [(40_000, 128, 64, 16384), (150_000, 16, 32, 4096), (20_000, 768, 32, 2048)])
def test_large_k_gpu_built_graphs(vg, ctx, kind, n, dim, r, k):
    base = rows(n, dim, 3 + kind)
    g, entry = gpu_graph(vg, ctx, base, r)
    idx, ov = make(vg, ctx, base, g, entry, kind, seed=kind)
    check(idx, ov, rows(4, dim, 11), k, kind)
    idx.close()


def test_k_at_least_n_and_unreachable_nodes(vg, ctx):
    """fewer than k results (k >= n; a graph whose second half is never reached): the rest padded"""
    n, dim = 1500, 16
    base = rows(n, dim, 21)
    g, entry = graphs.build_vamana(base, r=8, seed=3)
    for kind in (0, 1, 2, 3):
        idx, ov = make(vg, ctx, base, g, entry, kind, seed=kind)
        _, _, _, out = check(idx, ov, rows(3, dim, 5), 2000, kind)
        assert all(e[0].size <= n for e in out)
        idx.close()
    cut = g.copy()
    half = n // 2
    cut[cut >= half] = INVALID          # rows >= half: no edge leads there
    idx, ov = make(vg, ctx, base, cut, 0, 0)
    _, _, _, out = check(idx, ov, rows(3, dim, 6), 1024, 0)
    assert all(e[0].size <= half for e in out)
    idx, ov = make(vg, ctx, base, cut, 0, 2, metric=2)
    check(idx, ov, rows(3, dim, 6), 1024, 2, metric=2)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_filtered_large_k(vg, ctx, kind):
    n, dim, k = 6000, 32, 1500
    base = rows(n, dim, 40 + kind)
    g, entry = graphs.build_vamana(base, r=16, seed=4)
    idx, ov = make(vg, ctx, base, g, entry, kind, seed=kind)
    rng = np.random.default_rng(kind)
    q = rows(5, dim, 41)
    for keep in (0.3, 0.01):
        per_query = rng.random((5, n)) < keep
        per_query[1, entry] = False
        per_query[3, :] = False          # nothing passes: the walk visits the whole component
        check(idx, ov, q, k, kind, mask=per_query)
        check(idx, ov, q, k, kind, mask=per_query[0])
    # everything passes = the unfiltered search
    a = idx.search_vamana_filtered(q, k, np.ones(n, bool), kind=kind, stats=True)
    b = idx.search_vamana(q, k, kind=kind, stats=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])


def test_exploration_heap_past_65536(vg, ctx):
    """a walk whose exploration heap outgrows the 65 536 items the k <= 512 walk keeps: nothing may be dropped"""
    n, dim, r, k = 200_000, 16, 64, 16384
    rng = np.random.default_rng(77)
    base = rows(n, dim, 78)
    g = rng.integers(0, n, (n, r), dtype=np.uint32)      # a random 64-regular graph: every pop pushes many new nodes
    for kind in (0, 1):
        idx, ov = make(vg, ctx, base, g, 123, kind, seed=kind)
        ids, sc, st, out = check(idx, ov, rows(2, dim, 79), k, kind)
        est = out[0][2]
        assert est.nodes_visited - est.pops > 65536, (est.nodes_visited, est.pops)
        assert int(st[0][2]) == 0                       # no push dropped
        idx.close()


def test_chunked_batch(vg, ctx):
    """a batch split into several launches: under the test hook a launch has 64 MiB of scratch, and 150k rows at k = 4096 take
    (n + k) * 8 + n / 8 bytes per query, so 120 queries go in three launches"""
    n, dim, k = 150_000, 16, 4096
    base = rows(n, dim, 92)
    g, entry = gpu_graph(vg, ctx, base, 16)
    idx, ov = make(vg, ctx, base, g, entry, 0)
    q = rows(120, dim, 93)
    whole = idx.search_vamana(q, k, kind=0, stats=True)
    set_hook("VG_VAMANA_SMALL_SCRATCH", 1)
    try:
        ids, sc, st = idx.search_vamana(q, k, kind=0, stats=True)
    finally:
        set_hook("VG_VAMANA_SMALL_SCRATCH", 0)
    assert np.array_equal(ids, whole[0]) and np.array_equal(bits(sc), bits(whole[1])) and np.array_equal(st, whole[2])
    for qi in (0, 53, 60, 119):
        eid, esc, est = ov.search(q[qi], k)
        assert np.array_equal(ids[qi, :eid.size], eid) and np.array_equal(bits(sc[qi, :eid.size]), bits(esc)), qi
        assert (int(st[qi][0]), int(st[qi][1]), int(st[qi][3])) == (est.nodes_visited, est.distance_computations, est.pops), qi
    idx.close()


@pytest.mark.parametrize("k", [2048, 16384])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_nonfinite_inputs(vg, ctx, kind, k):
    """a NaN row, an Inf query and dot products that overflow: the queries at risk replay the reference's CandidateHeap"""
    n, dim = 20_000, 16
    base = rows(n, dim, 50)
    g, entry = gpu_graph(vg, ctx, base, 16)
    bad = base.copy()
    bad[17, 3] = np.nan
    bad[901, :] = np.nan
    q = rows(4, dim, 51)
    q[1, 2] = np.inf
    q[2] *= np.float32(3e19)             # squared terms and dot products beyond MaxFloat32
    for metric in ((0, 2) if kind == 0 else (0,)):
        idx, ov = make(vg, ctx, bad, g, entry, kind, metric=metric, seed=kind)
        check(idx, ov, q, k, kind, metric=metric)
        idx.close()
    if kind == 0:  # dot products that overflow both ways
        big = base * np.float32(1e19)
        idx, ov = make(vg, ctx, big, g, entry, 0, metric=2)
        check(idx, ov, rows(3, dim, 52) * np.float32(1e19), k, 0, metric=2)
        idx.close()


# ---- the threshold entry ------------------------------------------------------------------------------------------------------
def check_threshold(idx, ov, q, thr, max_results, kind, metric=0, mask=None):
    ids, sc, cnt, st = idx.search_vamana_threshold(q, thr, max_results, kind=kind, mask=mask, stats=True)
    for qi in range(q.shape[0]):
        mi = None if mask is None else (mask if mask.ndim == 1 else mask[qi])
        eid, esc, est = ov.search(q[qi], max_results, mask=mi)
        e_ids, e_sc, e_c = engine_filter(eid, esc, thr[qi], metric != 0, max_results)
        assert int(cnt[qi]) == e_c, (qi, thr[qi])
        assert np.array_equal(ids[qi], e_ids), qi
        assert same_scores(sc[qi], e_sc), qi
        assert (int(st[qi][0]), int(st[qi][1]), int(st[qi][3])) == (est.nodes_visited, est.distance_computations, est.pops)
    return ids, sc, cnt


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("max_results", [100, 3000, 16384])
def test_threshold_matches_engine_filter(vg, ctx, kind, metric, max_results):
    n, dim = 20_000, 32
    base = rows(n, dim, 60 + kind)
    base[::7] = base[3]                  # tied scores
    g, entry = gpu_graph(vg, ctx, base, 16)
    idx, ov = make(vg, ctx, base, g, entry, kind, metric, seed=kind)
    q = rows(7, dim, 61)
    ids, sc = idx.search_vamana(q, max_results, kind=kind)
    med = [sc[qi, min(max_results, n) // 3] for qi in range(7)]
    tie = sc[2, np.count_nonzero(ids[2] != INVALID) // 2]   # duplicate rows share this score: the boundary is kept
    thr = np.array([med[0], np.inf, tie, -np.inf, np.nan, med[5], med[6]], np.float32)
    check_threshold(idx, ov, q, thr, max_results, kind, metric)
    rng = np.random.default_rng(kind)
    m1 = rng.random(n) < 0.3
    mq = rng.random((7, n)) < 0.3
    check_threshold(idx, ov, q, thr, max_results, kind, metric, mask=m1)
    check_threshold(idx, ov, q, thr, max_results, kind, metric, mask=mq)
    idx.close()


def test_threshold_nan_scores_and_edges(vg, ctx):
    n, dim = 20_000, 16
    base = rows(n, dim, 70)
    g, entry = gpu_graph(vg, ctx, base, 16)
    bad = base.copy()
    bad[5] = np.nan
    for v in graphs_nan_neighbours(g, entry):
        bad[v, 0] = np.nan               # NaN scores inside the list
    q = rows(3, dim, 71)
    for metric in (0, 2):
        idx, ov = make(vg, ctx, bad, g, entry, 0, metric)
        for mr in (600, 4096):
            check_threshold(idx, ov, q, np.array([1e30, 30.0, np.nan], np.float32) * (1 if metric == 0 else -1), mr, 0, metric)
        # nq = 0 and max_results = 0: nothing is written
        ids, sc, cnt = idx.search_vamana_threshold(q[:0], np.zeros(0, np.float32), 1000, kind=0)
        assert ids.shape == (0, 1000) and cnt.shape == (0,)
        ids, sc, cnt = idx.search_vamana_threshold(q, np.zeros(3, np.float32), 0, kind=0)
        assert ids.shape == (3, 0)
        idx.close()


def graphs_nan_neighbours(g, entry):
    return [int(v) for v in g[entry][:4] if v != INVALID]


def test_refusals(vg, ctx):
    n, dim = 500, 16
    base = rows(n, dim, 80)
    g, entry = graphs.build_vamana(base, r=8, seed=1)
    idx, _ = make(vg, ctx, base, g, entry, 0)
    q = rows(2, dim, 81)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_vamana(q, 16385)
    assert e.value.status == -5 and "16384" in str(e.value)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_vamana_filtered(q, 16385, np.ones(n, bool))
    assert e.value.status == -5 and "16384" in str(e.value)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_vamana_threshold(q, np.zeros(2, np.float32), 16385)
    assert e.value.status == -5 and "16384" in str(e.value)
    idx.close()


def test_full_size_1m_x_768(vg, ctx):
    """1M x 768, a random 32-regular graph (search parity does not depend on graph quality), fp32 and PQ, 8 queries at k = 16384"""
    import torch
    n, dim, r, k, nq = 1_000_000, 768, 32, 16384, 8
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    base = torch.randn(n, dim, device="cuda", generator=gen)
    graph = np.random.default_rng(3).integers(0, n, (n, r), dtype=np.uint32)
    q = torch.randn(nq, dim, device="cuda", generator=gen)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    idx.set_vamana_graph(graph, 777)
    hbase, hq = base.cpu().numpy(), q.cpu().numpy()
    ids, sc, st = idx.search_vamana(q, k, kind=0, stats=True)
    ov = o.VamanaIndex(graph, 777, dim, o.VAMANA_F32, base=hbase)
    hid, hsc = ids.cpu().numpy().view(np.uint32), sc.cpu().numpy()
    for i in range(nq):
        eid, esc, est = ov.search(hq[i], k)
        assert np.array_equal(hid[i, :eid.size], eid) and np.array_equal(bits(hsc[i, :eid.size]), bits(esc)), i
        assert (int(st[i][0]), int(st[i][1]), int(st[i][3])) == (est.nodes_visited, est.distance_computations, est.pops), i
    pq = vg.ProductQuantizer(ctx, dim, 96, 256)
    pq.train(base[:20000], iters=3, seed=1)
    codes = pq.encode(base)
    idx.set_pq_codes(pq, codes)
    cb, s_, of_ = pq.codebooks()
    opq = o.ProductQuantizer(dim, 96, 256)
    opq.set_codebooks(cb, s_, of_)
    ids, sc, st = idx.search_vamana(q, k, kind=1, stats=True)
    ov = o.VamanaIndex(graph, 777, dim, o.VAMANA_PQ, pq=opq, codes=codes.cpu().numpy())
    hid, hsc = ids.cpu().numpy().view(np.uint32), sc.cpu().numpy()
    for i in range(nq):
        eid, esc, est = ov.search(hq[i], k)
        assert np.array_equal(hid[i, :eid.size], eid) and np.array_equal(bits(hsc[i, :eid.size]), bits(esc)), i
        assert (int(st[i][0]), int(st[i][1]), int(st[i][3])) == (est.nodes_visited, est.distance_computations, est.pops), i
    idx.close()
