"""Vamana construction on the GPU (vg_vamana_build) vs the sequential restatement of the header's rules
(tests/vamana_build_ref.py): the same graph, list order included, and the same entry point.  Then determinism,
the structure of a large build, search quality over the built graph, and the limits."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import vamana_build_ref as ref

pytestmark = pytest.mark.gpu

INVALID = ref.INVALID
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NOT_READY = -1, -5, -9


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def _index(vg, ctx, base, metric=0):
    idx = vg.Index(ctx, base.shape[0], base.shape[1], vg.Metric(metric))
    idx.set_vectors(base)
    return idx


def _data(kind, n, dim, rng):
    if kind == "normal":
        return rng.standard_normal((n, dim)).astype(np.float32)
    if kind == "grid":  # integer coordinates: many equal distances
        return rng.integers(0, 3, (n, dim)).astype(np.float32)
    if kind == "signs":  # {-1, 0, 1}: Dot products of -0 and many ties
        return rng.integers(-1, 2, (n, dim)).astype(np.float32)
    if kind == "dup":  # every row three times: zero distances
        return np.repeat(rng.standard_normal((n // 3 + 1, dim)).astype(np.float32), 3, axis=0)[:n]
    if kind == "nan":
        b = rng.standard_normal((n, dim)).astype(np.float32)
        b[n // 3, dim // 2] = np.nan
        return b
    raise ValueError(kind)


# (n, dim, metric, r, l, alpha, max_batch, growth_div, data)
SHAPES = [
    (300, 32, 0, 16, 40, 1.2, 1, 32, "normal"),      # sequential: the writer's loop
    (300, 32, 0, 16, 40, 1.2, 32, 4, "normal"),      # batches
    (600, 64, 0, 64, 100, 1.2, 64, 8, "normal"),     # NewWriter's defaults R 64, L 100, alpha 1.2
    (200, 768, 0, 16, 32, 1.2, 16, 4, "normal"),     # dim 768
    (300, 100, 2, 12, 30, 1.2, 16, 8, "normal"),     # ragged dim, Dot (raw, ascending)
    (300, 16, 1, 12, 30, 1.5, 1, 32, "normal"),      # Cosine = raw Dot as the writer sorts it; sequential
    (400, 8, 0, 8, 20, 1.2, 16, 8, "grid"),          # ties
    (300, 16, 0, 8, 20, 1.2, 8, 8, "dup"),           # duplicated rows: zero distances
    (9, 4, 0, 8, 10, 1.2, 1, 32, "normal"),          # n = r + 1: the complete graph to start from
    (1, 4, 0, 8, 10, 1.2, 1, 32, "normal"),          # n = 1
    (300, 16, 0, 8, 20, 1.2, 8, 8, "nan"),           # a NaN row: NaN distances sort last, the prune keeps them
    (300, 8, 2, 8, 20, 1.2, 8, 8, "signs"),          # Dot with -0 and ties
]


@pytest.mark.parametrize("n,dim,metric,r,l,alpha,max_batch,growth_div,data", SHAPES)
def test_parity(vg, ctx, n, dim, metric, r, l, alpha, max_batch, growth_div, data):
    rng = np.random.default_rng(n * 31 + dim + metric)
    base = _data(data, n, dim, rng)
    idx = _index(vg, ctx, base, metric)
    idx.build_vamana(r=r, l=l, alpha=alpha, seed=5, max_batch=max_batch, growth_div=growth_div)
    g, entry = idx.get_vamana_graph()
    eg, eentry = ref.build(base, metric, r, l, alpha, seed=5, max_batch=max_batch, growth_div=growth_div)
    assert entry == eentry
    bad = np.nonzero((g != eg).any(1))[0]
    assert bad.size == 0, (bad[:5], g[bad[0]], eg[bad[0]])


def test_parity_init_graph_with_empty_slots(vg, ctx):
    rng = np.random.default_rng(3)
    n, dim, r = 200, 16, 8
    base = rng.standard_normal((n, dim)).astype(np.float32)
    init = np.full((n, r), INVALID, np.uint32)
    for i in range(n):
        ids = [j for j in rng.choice(n, size=r, replace=False).tolist() if j != i]
        slots = sorted(rng.choice(r, size=len(ids), replace=False).tolist())[: int(rng.integers(0, len(ids) + 1))]
        for s, j in zip(slots, ids):
            init[i, s] = j
    idx = _index(vg, ctx, base)
    idx.build_vamana(r=r, l=20, alpha=1.2, init_graph=init, max_batch=8, growth_div=8)
    g, entry = idx.get_vamana_graph()
    eg, eentry = ref.build(base, 0, r, 20, 1.2, init_graph=init, max_batch=8, growth_div=8)
    assert entry == eentry and np.array_equal(g, eg)


def test_deterministic(vg, ctx):
    rng = np.random.default_rng(8)
    base = rng.standard_normal((50_000, 128)).astype(np.float32)
    idx = _index(vg, ctx, base)
    idx.build_vamana(r=32, l=64, alpha=1.2)
    g1, e1 = idx.get_vamana_graph()
    idx.build_vamana(r=32, l=64, alpha=1.2)
    g2, e2 = idx.get_vamana_graph()
    assert e1 == e2 and np.array_equal(g1, g2)


def test_structure_100k_768(vg, ctx):
    rng = np.random.default_rng(9)
    n, r = 100_000, 64
    base = rng.standard_normal((n, 768)).astype(np.float32)
    idx = _index(vg, ctx, base)
    idx.build_vamana()
    g, entry = idx.get_vamana_graph()
    assert g.shape == (n, r)
    _, eentry = ref.centroid_entry(base, 0)
    assert entry == eentry
    valid = g != INVALID
    assert (g[valid] < n).all()
    assert not (g == np.arange(n, dtype=np.uint32)[:, None]).any()
    s = np.sort(np.where(valid, g, INVALID).astype(np.int64), axis=1)
    assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] != INVALID)).any()
    assert valid.sum(1).min() >= 1
    # the valid ids of each row come first
    assert not (~valid[:, :-1] & valid[:, 1:]).any()


def _recall(ids, truth):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / truth.shape[1] for a, b in zip(ids, truth)]))


def test_quality_20k(vg, ctx):
    rng = np.random.default_rng(12)
    n, dim, k = 20_000, 128, 10
    centers = rng.standard_normal((64, dim)).astype(np.float32) * 4
    base = (centers[rng.integers(0, 64, n)] + rng.standard_normal((n, dim))).astype(np.float32)
    queries = (centers[rng.integers(0, 64, 1000)] + rng.standard_normal((1000, dim))).astype(np.float32)
    idx = _index(vg, ctx, base)
    truth, _ = idx.search_flat(queries, k)
    idx.build_vamana(r=32, l=64, alpha=1.2)
    g, entry = idx.get_vamana_graph()
    built = _recall(idx.search_vamana(queries, k)[0], truth)
    idx.set_vamana_graph(np.array(ref.initial_graph(n, 32, 0), np.uint32), entry)
    rand = _recall(idx.search_vamana(queries, k)[0], truth)
    # batched against the writer's sequential loop on the first 5000 rows (the sequential build is one node per batch)
    sub = _index(vg, ctx, base[:5000])
    sub_truth, _ = sub.search_flat(queries, k)
    sub.build_vamana(r=32, l=64, alpha=1.2)
    sub_built = _recall(sub.search_vamana(queries, k)[0], sub_truth)
    sub.build_vamana(r=32, l=64, alpha=1.2, max_batch=1)
    seq = _recall(sub.search_vamana(queries, k)[0], sub_truth)
    print(f"recall@10: built {built:.4f}, initial random graph {rand:.4f}; 5000 rows: batched {sub_built:.4f}, sequential {seq:.4f}")
    # measured on MI355X: built 0.346, initial random graph 0.024; 5000 rows: batched 0.904, sequential 0.906.  The
    # writer's search stops at its first l + 50 pool entries, and at 20k rows its graph is what limits recall (the
    # sequential build, the reference's own loop, measures the same 0.342)
    assert built >= 0.30
    assert built >= rand + 0.25
    assert sub_built >= 0.85
    assert abs(sub_built - seq) <= 0.02


def test_round_trip_and_reference_writer_search(vg, ctx):
    base = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0]], np.float32)
    idx = _index(vg, ctx, base)
    idx.build_vamana(r=4, l=10, alpha=1.2)
    g, entry = idx.get_vamana_graph()
    eg, eentry = ref.build(base, 0, 4, 10, 1.2)
    assert entry == eentry and np.array_equal(g, eg)
    ids, scores = idx.search_vamana(base[:1], 2)  # writer_test.go:115-129: the query finds row 0 at score 0
    assert ids[0, 0] == 0 and scores[0, 0] == 0.0
    other = _index(vg, ctx, base)
    other.set_vamana_graph(g, entry)
    g2, e2 = other.get_vamana_graph()
    assert e2 == entry and np.array_equal(g2, g)


def test_limits(vg, ctx):
    base = np.random.default_rng(1).standard_normal((50, 8)).astype(np.float32)
    idx = _index(vg, ctx, base)
    for kw, status, word in [({"r": 65}, ERR_UNSUPPORTED, "65"), ({"l": 1025}, ERR_UNSUPPORTED, "1025"),
                             ({"max_batch": 0}, ERR_INVALID_ARG, "max_batch")]:
        with pytest.raises(vg.VecgoHipError) as e:
            idx.build_vamana(**kw)
        assert e.value.status == status and word in e.value.message
    bad = np.full((50, 8), INVALID, np.uint32)
    bad[7, 2] = 7
    with pytest.raises(vg.VecgoHipError) as e:
        idx.build_vamana(r=8, init_graph=bad)
    assert e.value.status == ERR_INVALID_ARG and "itself" in e.value.message
    bad[7, 2] = 50
    with pytest.raises(vg.VecgoHipError) as e:
        idx.build_vamana(r=8, init_graph=bad)
    assert e.value.status == ERR_INVALID_ARG
    bad[7, 2] = 3
    bad[7, 5] = 3
    with pytest.raises(vg.VecgoHipError) as e:
        idx.build_vamana(r=8, init_graph=bad)
    assert e.value.status == ERR_INVALID_ARG and "twice" in e.value.message
    bare = vg.Index(ctx, 50, 8)
    with pytest.raises(vg.VecgoHipError) as e:
        bare.build_vamana()
    assert e.value.status == ERR_NOT_READY and "fp32" in e.value.message
    empty = vg.Index(ctx, 0, 8)
    with pytest.raises(vg.VecgoHipError) as e:
        empty.build_vamana()
    assert e.value.status == ERR_INVALID_ARG and "no vectors" in e.value.message
