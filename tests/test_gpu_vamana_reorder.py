"""vg_vamana_reorder_bfs on the GPU against the writer's reorderBFS restated (tests/reorder_bfs_ref.py): the same
permutation, graph and entry point bit for bit; an index reordered in place searches exactly like one built fresh from
the permuted host arrays (and like the DiskANN segment the writer would flush); searches map through inv_perm; a
second reorder is the identity; refusals change nothing."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks, reorder_bfs_ref as ref, segfile

pytestmark = pytest.mark.gpu

X = ref.INVALID
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NOT_READY = -1, -5, -9


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _check_reorder(vg, ctx, idx, g, entry):
    want = ref.reorder_np(g, entry)
    perm, inv = idx.reorder_vamana_bfs()
    ng, ne = idx.get_vamana_graph()
    assert np.array_equal(perm, want[0]) and np.array_equal(inv, want[1])
    assert np.array_equal(ng, want[2]) and ne == want[3]
    return perm, inv


def _graph_index(vg, ctx, g, entry, dim=4):
    idx = vg.Index(ctx, g.shape[0], dim)
    idx.set_vamana_graph(g, entry)
    return idx


@pytest.mark.parametrize("r,metric", [(32, 0), (64, 2)])
def test_built_graph(vg, ctx, r, metric):
    rng = np.random.default_rng(r)
    n, dim = 20000, 128
    base = rng.standard_normal((n, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(base)
    idx.build_vamana(r=r, l=64, seed=3)
    g, entry = idx.get_vamana_graph()
    _check_reorder(vg, ctx, idx, g, entry)


def test_sparse_in_degree_graph(vg, ctx):
    # random lists with holes mid-list; about 10 % of the nodes are listed by no one; the entry in the middle
    rng = np.random.default_rng(7)
    n, r = 30000, 16
    listed = np.flatnonzero(rng.random(n) >= 0.1)
    g = listed[rng.integers(0, listed.size, (n, r))].astype(np.uint32)
    g[rng.random((n, r)) < 0.15] = X
    _check_reorder(vg, ctx, _graph_index(vg, ctx, g, int(listed[listed.size // 2])), g, int(listed[listed.size // 2]))


@pytest.mark.parametrize("shape", ["path", "path_back", "empty", "ladder"])
def test_degenerate_graphs(vg, ctx, shape):
    n, r = 100000, 4
    g = np.full((n, r), X, np.uint32)
    entry = 0
    if shape == "path":        # depth n
        g[:-1, 0] = np.arange(1, n)
    elif shape == "path_back":  # both directions, entry in the middle, ids in the last slot
        g[:-1, 3] = np.arange(1, n)
        g[1:, 1] = np.arange(0, n - 1)
        entry = n // 2
    elif shape == "ladder":    # levels of 700 nodes (wider than one workgroup walks), then the tail
        w = 700
        for s in range(4):
            g[: n - w, s] = (np.arange(n - w) + w + s * 7) % n
        g[n // 2:] = X
        entry = 3
    _check_reorder(vg, ctx, _graph_index(vg, ctx, g, entry), g, entry)


def _coded_index(vg, ctx, base, pq, pq_codes, rq_codes, iq, i4_codes, sq, sq_codes, g, entry):
    n, dim = base.shape
    idx = vg.Index(ctx, n, dim, vg.Metric.L2)
    idx.set_vectors(base)
    idx.enable_bf16_filter(True)
    idx.set_pq_codes(pq, pq_codes)
    idx.enable_pq_nomination(True)
    idx.set_rabitq_codes(rq_codes)
    idx.set_int4_codes(iq, i4_codes)
    idx.set_sq8_codes(sq, sq_codes)
    idx.enable_sq8_nomination(True)
    idx.set_vamana_graph(g, entry)
    return idx


def _all_searches(idx, q, k=10):
    out = [idx.search_vamana(q, k, kind=kind) for kind in range(4)]
    out.append(idx.search_flat(q, k))
    hooks.set_hook("VG_PQ_NOM_ALWAYS", 1)
    try:
        out.append(idx.search_pq_adc(q, k))
    finally:
        hooks.set_hook("VG_PQ_NOM_ALWAYS", 0)
    out.append(idx.search_sq8(q, k))
    out.append(idx.search_rabitq(q, k))
    return out


def test_reordered_index_equals_fresh_index_of_permuted_arrays(vg, ctx):
    rng = np.random.default_rng(21)
    n, dim, r, nq = 6000, 64, 24, 160
    base = np.floor(rng.standard_normal((n, dim)) * 4).astype(np.float32)  # coarse rows: ties among the scores
    q = np.floor(rng.standard_normal((nq, dim)) * 4).astype(np.float32)
    pq = vg.ProductQuantizer(ctx, dim, 16, 256)
    pq.train(base[:1500], iters=4, seed=5)
    pq_codes = pq.encode(base)
    rq_codes = o.rabitq_encode_batch(base, dim)
    iq = vg.Int4Quantizer(ctx, dim)
    iq.train(base)
    oi = o.Int4Quantizer(dim)
    oi.train(base)
    i4_codes = oi.encode_batch(base)
    sq = vg.ScalarQuantizer(ctx, dim)
    sq.train(base)
    sq_codes = sq.encode(base)
    g = rng.integers(0, n, (n, r)).astype(np.uint32)
    g[rng.random((n, r)) < 0.3] = X
    entry = n // 3
    idx = _coded_index(vg, ctx, base, pq, pq_codes, rq_codes, iq, i4_codes, sq, sq_codes, g, entry)
    perm, inv = idx.reorder_vamana_bfs()
    want = ref.reorder_np(g, entry)
    assert np.array_equal(perm, want[0])
    fresh = _coded_index(vg, ctx, base[perm], pq, pq_codes[perm], rq_codes[perm], iq, i4_codes[perm], sq, sq_codes[perm],
                         want[2], want[3])
    for i, (a, b) in enumerate(zip(_all_searches(idx, q), _all_searches(fresh, q))):
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), i
    # the DiskANN segment the writer would flush from the permuted arrays (PQ codes, then INT4 codes)
    cb, sc, of = pq.codebooks()
    for extra, kinds in ((dict(pq=(16, 256, sc, of, cb), pq_codes=pq_codes[perm]), (0, 1)),
                         (dict(int4=(oi.min, oi.diff, i4_codes[perm])), (0, 3))):
        seg = vg.Segment(ctx, segfile.write_diskann(base[perm], want[2], want[3], **extra), kind="diskann")
        for kind in kinds:
            a, b = idx.search_vamana(q, 10, kind=kind), seg.index.search_vamana(q, 10, kind=kind)
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), kind


def test_search_maps_through_inv_perm_and_second_reorder_is_identity(vg, ctx):
    rng = np.random.default_rng(5)
    n, dim = 8000, 32
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((64, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    idx.build_vamana(r=16, l=40, seed=9)
    ids0, sc0 = idx.search_vamana(q, 10)
    perm, inv = idx.reorder_vamana_bfs()
    ids1, sc1 = idx.search_vamana(q, 10)
    assert np.array_equal(ids1, inv[ids0]) and np.array_equal(bits(sc1), bits(sc0))
    g1, e1 = idx.get_vamana_graph()
    p2, i2 = idx.reorder_vamana_bfs()
    assert np.array_equal(p2, np.arange(n)) and np.array_equal(i2, np.arange(n))
    g2, e2 = idx.get_vamana_graph()
    assert np.array_equal(g1, g2) and e1 == e2 == 0
    ids2, sc2 = idx.search_vamana(q, 10)
    assert np.array_equal(ids2, ids1) and np.array_equal(bits(sc2), bits(sc1))


def test_refusals_change_nothing(vg, ctx):
    import ctypes as C
    from vecgo_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    n, dim = 500, 16
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((8, dim)).astype(np.float32)
    sentinel = np.full(n, 7, np.uint32)

    def call(idx):
        p, i = sentinel.copy(), sentinel.copy()
        st = lib.vg_vamana_reorder_bfs(idx._h, C.c_void_p(p.ctypes.data), C.c_void_p(i.ctypes.data), None)
        assert np.array_equal(p, sentinel) and np.array_equal(i, sentinel)
        return st

    plain = vg.Index(ctx, n, dim)
    plain.set_vectors(base)
    before = plain.search_flat(q, 5)
    assert call(plain) == ERR_NOT_READY
    after = plain.search_flat(q, 5)
    assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1]))

    g = rng.integers(0, n, (n, 8)).astype(np.uint32)
    for setup in ("hnsw", "partitions"):
        idx = vg.Index(ctx, n, dim)
        idx.set_vectors(base)
        if setup == "hnsw":
            idx.build_hnsw(m=8, ef_construction=32)
        else:
            idx.set_partitions(base[:2].copy(), np.array([0, 250, n], np.uint32))
        idx.set_vamana_graph(g, 5)
        vb = idx.search_vamana(q, 5)
        assert call(idx) == ERR_UNSUPPORTED
        va = idx.search_vamana(q, 5)
        assert np.array_equal(vb[0], va[0]) and np.array_equal(bits(vb[1]), bits(va[1]))
        assert np.array_equal(idx.get_vamana_graph()[0], g) and idx.get_vamana_graph()[1] == 5
    assert lib.vg_vamana_reorder_bfs(None, None, None, None) == ERR_INVALID_ARG
    empty = vg.Index(ctx, 0, dim)
    empty.set_vamana_graph(np.zeros((0, 8), np.uint32), 0)
    assert empty.reorder_vamana_bfs()[0].size == 0
