"""Every node scorer of the HNSW walk (F32ScorerT, PqScorerT<DIRECT> of vg_node_score.hpp) under every heap and extraction form
of hnsw_search_kernel (k_graph.hip), against the oracle's walk over the same graph: ids, score bits, padding and the
(nodes_visited, distance_computations, distance_short_circuits, pops) counters.  The HNSW counterpart of
test_gpu_vamana_scorers.py.

The shapes are the ones at which a scorer takes another path:
  fp32        dim 20 (one partial 16-lane pass) and 100 (ragged tail); L2, Cosine over normalised rows, Dot (UK = false)
  PQ table    any sub-dimension but 8 — the four hnsw_search_kernel<1, ...> instances, the per-launch BuildDistanceTable image:
              m = 8 and 12 (scalar loop only; sub-dimensions 4 and 3), 16 (one 16-group), 48 (32-chunk + 16-chunk), 96 (the 96-chunk),
              3 and 5 (sub-dimension 16, odd m)
  PQ direct   sub-dimension 8: m = 3 (pair + odd scalar tail), 5, 16 (one 16-group), 48 (32-chunk + 16-chunk)
(k, ef): the heaps of a walk live in LDS up to ef = VG_PQ_LDS_HEAPS_MAX = 448 (PQ) / kHnswLdsEf = 512 (fp32) — the defaults in
k_graph.hip — and are split between LDS and HBM above; k < 64 is extracted by the register selection, k >= 64 by the LDS sort
(LDS heaps) or the pops (split heaps).
Each (scorer, k, ef) runs plain; with an Inf in one coordinate of one query (the STRICT pass answers it: for the table form over a
table that itself holds Inf / NaN); and over a graph with 40 % tombstones (every query takes the STRICT instance, which reads the
bitmap)."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import graphs
from tests.test_gpu_graph import bits
from tests.test_gpu_vamana_large_k import same_scores

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


N, M, NQ = 700, 8, 6
F32 = [("f32", 20, 0), ("f32", 100, 0), ("f32", 20, 1), ("f32", 20, 2)]          # arg: the metric (L2, Cosine, Dot)
PQ_TABLE = [("pq", 32, 8), ("pq", 36, 12), ("pq", 64, 16), ("pq", 192, 48), ("pq", 384, 96), ("pq", 48, 3), ("pq", 80, 5)]  # arg: m
PQ_DIRECT = [("pq", 24, 3), ("pq", 40, 5), ("pq", 128, 16), ("pq", 384, 48)]
SCORERS = F32 + PQ_TABLE + PQ_DIRECT
# LDS heaps + register selection; LDS heaps + LDS sort; LDS heaps for both walks; split for PQ only; split for both; split with k >= 64
KEF = [(10, 64), (70, 128), (10, 448), (10, 449), (10, 513), (100, 600)]

_cases = {}


def random_pq(vg, ctx, rng, dim, m):
    """(GPU quantizer, oracle quantizer) with the same random int8 codebooks: no training"""
    sub = dim // m
    opq = o.ProductQuantizer(dim, m, 256)
    opq.set_codebooks(rng.integers(-128, 128, m * 256 * sub).astype(np.int8), (rng.random(m) * 0.02 + 0.005).astype(np.float32),
                      ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32))
    pq = vg.ProductQuantizer(ctx, dim, m, 256)
    pq.set_codebooks(opq.codebooks, opq.scales, opq.offsets)
    return pq, opq


def case(vg, ctx, scorer, dim, arg):
    """(GPU index, oracle walk, the GPU search, queries, tombstones) of one scorer shape, built once and left unchanged.
    arg: the metric (fp32) or m (PQ)"""
    key = (scorer, dim, arg)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(1000 * dim + 10 * arg + (scorer == "pq"))
    metric = arg if scorer == "f32" else 0
    base = rng.standard_normal((N, dim)).astype(np.float32)
    q = rng.standard_normal((NQ, dim)).astype(np.float32)
    if metric == 1:
        base /= np.linalg.norm(base, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    # (the graph's construction is not under test: near neighbours by the first 32 coordinates keep the set-up short)
    l0, upper, entry = graphs.build_hnsw(base[:, :min(dim, 32)], m=M, seed=dim)
    assert len(upper) > 0                                    # the greedy descent (sc.one, greedy_layer) runs through the scorer too
    idx = vg.Index(ctx, N, dim, vg.Metric(metric))
    idx.set_vectors(base)
    idx.set_hnsw_graph(l0, upper, entry, m=M)
    if scorer == "f32":
        oidx = o.HnswIndex(base, dim, l0, upper, entry, metric=metric)
        search = idx.search_hnsw
    else:
        pq, opq = random_pq(vg, ctx, rng, dim, arg)
        codes = opq.encode_batch(base)
        idx.set_pq_codes(pq, codes)
        oidx = o.HnswIndex(base, dim, l0, upper, entry, metric=metric, pq=opq, codes=codes)
        search = idx.search_hnsw_pq
    dead = rng.random(N) < 0.4
    _cases[key] = (idx, oidx, search, q, dead)
    return _cases[key]


def stats_tuple(st):
    return (st.nodes_visited, st.distance_computations, st.distance_short_circuits, st.pops)


def compare(got, want, queries):
    """got: (ids, scores, stats) of a batch; want(qi): the oracle's (ids, scores, stats) of query qi, for each qi in `queries`"""
    ids, sc, st = got
    out = {}
    for qi in queries:
        eid, esc, est = want(qi)
        r = eid.size
        assert np.array_equal(ids[qi, :r], eid), (qi, ids[qi], eid)
        assert same_scores(sc[qi, :r], esc), qi
        assert np.all(ids[qi, r:] == INVALID), (qi, r)
        assert tuple(int(x) for x in st[qi]) == stats_tuple(est), (qi, st[qi], stats_tuple(est))
        out[qi] = (eid, esc, est)
    return out


def check(search, oidx, q, k, ef):
    """search(q, k, ef, stats=True) against the oracle's walk, query by query"""
    got = search(q, k, ef, stats=True)
    assert got[0].shape == (q.shape[0], k) and got[1].shape == (q.shape[0], k)
    return got + (compare(got, lambda qi: oidx.search(q[qi], k, ef), range(q.shape[0])),)


@pytest.mark.parametrize("k,ef", KEF)
@pytest.mark.parametrize("scorer,dim,arg", SCORERS)
def test_scorer_under_every_heap_form(vg, ctx, scorer, dim, arg, k, ef):
    idx, oidx, search, q, dead = case(vg, ctx, scorer, dim, arg)
    check(search, oidx, q, k, ef)


@pytest.mark.parametrize("k,ef", KEF)
@pytest.mark.parametrize("scorer,dim,arg", SCORERS)
def test_strict_pass_answers_an_inf_query(vg, ctx, scorer, dim, arg, k, ef):
    """one query in six with an Inf in one coordinate: the PQ walks flag it in the query check up front, the fp32 walks by their
    NaN watch, and the STRICT pass (float comparisons, the reference's heaps as written) answers it — the table form over a table
    that holds Inf / NaN; the other five return from that pass at once"""
    idx, oidx, search, q, dead = case(vg, ctx, scorer, dim, arg)
    q = q.copy()
    q[2, dim // 3] = np.inf
    assert oidx.search(q[2], k, ef)[2].pops >= 1             # the oracle answers this input
    check(search, oidx, q, k, ef)


@pytest.mark.parametrize("k,ef", KEF)
@pytest.mark.parametrize("scorer,dim,arg", SCORERS)
def test_strict_pass_reads_the_tombstones(vg, ctx, scorer, dim, arg, k, ef):
    """40 % of the rows deleted: every query takes the STRICT instance, which walks through deleted nodes and returns none"""
    idx, oidx, search, q, dead = case(vg, ctx, scorer, dim, arg)
    oidx.set_tombstones(dead)
    idx.set_hnsw_tombstones(dead)
    try:
        ids = check(search, oidx, q, k, ef)[0]
        assert not dead[ids[ids != INVALID]].any()
    finally:                                                 # (the case is cached)
        oidx.set_tombstones(None)
        idx.set_hnsw_tombstones(None)


# ---- ties on the table form -----------------------------------------------------------------------------------------------------
_grids = {}


def grid_case(vg, ctx, grid):
    """test_hnsw_duplicate_distances' integer grid (tests/test_gpu_graph.py) scored from PQ codes with m = 2 (sub-dimension 4: the
    table form), the centroids drawn from the grid: quantised sums tie heavily"""
    if grid in _grids:
        return _grids[grid]
    rng = np.random.default_rng(5 + grid)
    n = 1500
    pts = rng.integers(0, grid, (n, 8)).astype(np.float32)
    l0, upper, entry = graphs.build_hnsw(pts, m=8, seed=3)
    q = rng.integers(0, grid, (16, 8)).astype(np.float32)
    cb = rng.integers(0, grid, 2 * 256 * 4).astype(np.int8)  # centroids on the grid itself: every table entry is a small integer
    scales = np.ones(2, np.float32)
    offsets = np.zeros(2, np.float32)
    opq = o.ProductQuantizer(8, 2, 256); opq.set_codebooks(cb, scales, offsets)
    pq = vg.ProductQuantizer(ctx, 8, 2, 256); pq.set_codebooks(cb, scales, offsets)
    codes = opq.encode_batch(pts)
    idx = vg.Index(ctx, n, 8)
    idx.set_vectors(pts)
    idx.set_hnsw_graph(l0, upper, entry, m=8)
    idx.set_pq_codes(pq, codes)
    oq = o.HnswIndex(pts, 8, l0, upper, entry, m=8, pq=opq, codes=codes)
    _grids[grid] = (idx, oq, q)
    return _grids[grid]


@pytest.mark.parametrize("k,ef", [(10, 32), (64, 64), (100, 300), (10, 600), (70, 700)])
@pytest.mark.parametrize("grid", [3, 40])   # 3: nearly every distance tied; 40: a tie here and there
def test_table_form_duplicate_distances(vg, ctx, k, ef, grid):
    """many equal PQ distances: the heaps' tie behaviour decides which ids survive and in which order they come out, and the
    selection falls back to the pops when the k + 1 closest tie"""
    idx, oq, q = grid_case(vg, ctx, grid)
    kk = min(k, ef)
    out = check(idx.search_hnsw_pq, oq, q, kk, ef)[3]
    if grid == 3:                                            # the case is about ties: every query's list holds equal scores
        assert all(np.unique(bits(esc)).size < esc.size for _, esc, _ in out.values())


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_hnsw_pq_refusals(vg, ctx):
    """vg_search_hnsw_pq's refusals that no other test names.  The Python layer passes its arguments straight through: each of
    these is refused by the library (search_hnsw_impl, k_graph.hip), before any scratch is taken."""
    rng = np.random.default_rng(3)
    n, dim = 200, 16
    base = rng.standard_normal((n, dim)).astype(np.float32)
    l0, upper, entry = graphs.build_hnsw(base, m=4, seed=1)
    q = base[:2]

    def index(metric=0):
        idx = vg.Index(ctx, n, dim, vg.Metric(metric))
        idx.set_vectors(base)
        idx.set_hnsw_graph(l0, upper, entry, m=4)
        return idx

    pq, opq = random_pq(vg, ctx, rng, dim, 4)
    codes = opq.encode_batch(base)

    # a quantizer with 16 centroids (the walk's table and codebook forms are written for 256)
    pq16 = vg.ProductQuantizer(ctx, dim, 4, 16)
    pq16.set_codebooks(rng.integers(-128, 128, 4 * 16 * 4).astype(np.int8), np.full(4, 0.01, np.float32), np.zeros(4, np.float32))
    idx = index()
    idx.set_pq_codes(pq16, rng.integers(0, 16, (n, 4)).astype(np.uint8))
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_hnsw_pq(q, 3, 10)
    assert e.value.status == -5 and "numCentroids == 256" in e.value.message
    idx.close()

    # a metric other than L2: ComputeAsymmetricDistance is an L2 distance
    for metric in (1, 2):
        idx = index(metric)
        idx.set_pq_codes(pq, codes)
        with pytest.raises(vg.VecgoHipError) as e:
            idx.search_hnsw_pq(q, 3, 10)
        assert e.value.status == -5 and "metric must be L2" in e.value.message
        idx.close()

    # a graph and rows, but no PQ codes
    idx = index()
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_hnsw_pq(q, 3, 10)
    assert e.value.status == -9 and "PQ codes" in e.value.message

    # ef above 1 << 20 (kHnswMaxEf)
    idx.set_pq_codes(pq, codes)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_hnsw_pq(q, 3, (1 << 20) + 1)
    assert e.value.status == -5 and "exceeds" in e.value.message
    ids, sc = idx.search_hnsw_pq(q, 3, 10)                   # and the index answers what it is asked within the limits
    for qi in range(2):
        eid, esc, _ = o.HnswIndex(base, dim, l0, upper, entry, m=4, pq=opq, codes=codes).search(q[qi], 3, 10)
        assert np.array_equal(ids[qi, :eid.size], eid) and same_scores(sc[qi, :eid.size], esc)
    idx.close()
