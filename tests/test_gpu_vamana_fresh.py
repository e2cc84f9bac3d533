"""The streaming Vamana index on the GPU (vg_vamana_insert, vg_search_vamana_fresh) vs the sequential restatement of the
header's rules (tests/vamana_fresh_ref.py): the same graph bit for bit, list order included, the same entry point, the
same search ids and score bits.  Then the reference's recall floor and the limits."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import vamana_fresh_ref as ref

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


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _data(kind, n, dim, rng):
    if kind == "normal":
        return rng.standard_normal((n, dim)).astype(np.float32)
    if kind == "grid":  # integer coordinates: many equal distances
        return rng.integers(0, 3, (n, dim)).astype(np.float32)
    if kind == "dup":  # every row three times: zero distances, ties in arrival order
        return np.repeat(rng.standard_normal((n // 3, dim)).astype(np.float32), 3, axis=0)
    if kind == "hub":  # row 0 is nearer to every row than any other row is: every new list begins with it
        b = rng.standard_normal((n, dim)).astype(np.float32)
        b[0] = 0
        return b
    if kind == "nan":
        b = rng.standard_normal((n, dim)).astype(np.float32)
        b[n // 3, dim // 2] = np.nan
        return b
    raise ValueError(kind)


def _same_graph(idx, graph, entry, r):
    g, e = idx.get_vamana_graph()
    eg = ref.array_of(graph, r)
    assert g.shape == eg.shape
    bad = np.nonzero((g != eg).any(1))[0]
    assert bad.size == 0, (bad[:5], g[bad[0]], eg[bad[0]])
    assert e == entry
    return g


def _valid_lists(g, n):
    for i, row in enumerate(g):
        ids = row[row != INVALID]
        assert (row[:ids.size] != INVALID).all(), i  # a dense prefix
        assert (ids < n).all() and np.unique(ids).size == ids.size and i not in ids, i


# rows 1-9 of the issue's table, from an empty index: (n, dim, metric, r, l, alpha, max_batch, growth_div, data)
FROM_EMPTY = [
    (300, 32, 0, 16, 40, 1.2, 1, 32, "normal"),     # the serial loop, crossing count 100
    (300, 32, 0, 16, 40, 1.2, 32, 4, "normal"),     # batches
    (600, 64, 0, 0, 0, 0.0, 64, 8, "normal"),       # the defaults: R 64, L 100, alpha 1.2
    (200, 768, 0, 16, 32, 1.2, 16, 4, "normal"),    # dim 768
    (300, 100, 2, 12, 30, 1.2, 16, 8, "normal"),    # ragged dim, Dot (raw, ascending)
    (300, 16, 1, 12, 30, 1.5, 1, 32, "normal"),     # Cosine = raw Dot; alpha 1.5
    (400, 8, 0, 8, 20, 1.2, 16, 8, "grid"),         # ties, and the reverse-edge prune at a full list
    (300, 16, 0, 8, 20, 1.2, 8, 8, "dup"),          # zero distances and arrival-order ties
    (150, 16, 0, 16, 1024, 1.2, 8, 8, "normal"),    # results never fills: the walk runs dry
    (300, 16, 0, 8, 20, 1.2, 8, 8, "nan"),          # a NaN row: after +Inf, in arrival order
    (2000, 32, 0, 8, 20, 1.2, 1024, 1, "hub"),      # batches that double up to 977 nodes, all linking the hub row
]


@pytest.mark.parametrize("n,dim,metric,r,l,alpha,max_batch,growth_div,data", FROM_EMPTY)
def test_insert_from_empty(vg, ctx, n, dim, metric, r, l, alpha, max_batch, growth_div, data):
    rng = np.random.default_rng(n * 31 + dim + metric)
    base = _data(data, n, dim, rng)
    idx = vg.Index(ctx, 0, dim, vg.Metric(metric))
    idx.insert_vamana(base, r=r, l=l, alpha=alpha, seed=3, max_batch=max_batch, growth_div=growth_div)
    assert idx.n == n
    graph, entry = ref.insert(base, 0, metric=metric, r=r, l=l, alpha=alpha, seed=3, max_batch=max_batch, growth_div=growth_div)
    if data == "grid":
        assert ref.STATS["full_prunes"] > 0  # the case is about reverse edges into full lists
    if data == "hub":
        assert ref.STATS["max_records"] > 256  # more records for one target than its workgroup has threads
    g = _same_graph(idx, graph, entry, r or ref.DEFAULT_R)
    _valid_lists(g, n)
    # the walk of the query search over the same graph: ids and score bits
    q = base[rng.choice(n, 8, replace=False)] if data != "nan" else base[[n // 3, 0, 1]]
    ids, sc, cnt = idx.search_vamana_fresh(q, 5, l=l)
    eids, esc, ecnt = ref.search(base, graph, entry, q, 5, l=l, metric=metric)
    assert np.array_equal(cnt, ecnt) and np.array_equal(ids, eids) and np.array_equal(_bits(sc), _bits(esc))


def _built(vg, ctx, base, r, l):
    idx = vg.Index(ctx, base.shape[0], base.shape[1], vg.Metric(0))
    idx.set_vectors(base)
    idx.build_vamana(r=r, l=l, alpha=1.2, seed=5, max_batch=16, growth_div=8)
    g, e = idx.get_vamana_graph()
    return idx, g, e


def test_insert_into_built_graph(vg, ctx):  # row 10a
    rng = np.random.default_rng(10)
    base = rng.standard_normal((400, 16)).astype(np.float32)
    idx, g0, e0 = _built(vg, ctx, base[:300], 16, 40)
    idx.insert_vamana(base[300:], r=16, l=40, max_batch=8, growth_div=8)
    graph, entry = ref.insert(base, 300, ref.lists_of(g0), e0, r=16, l=40, max_batch=8, growth_div=8)
    _valid_lists(_same_graph(idx, graph, entry, 16), 400)


def test_insert_into_uploaded_graph_with_holes(vg, ctx):  # row 10b
    rng = np.random.default_rng(11)
    base = rng.standard_normal((300, 16)).astype(np.float32)
    r = 8
    g0 = np.full((200, r), INVALID, np.uint32)
    for i in range(200):  # random lists with empty slots in mid-list; some full
        ids = [j for j in rng.choice(200, size=r + 1, replace=False).tolist() if j != i][:r]
        keep = r if i % 4 == 0 else int(rng.integers(0, r + 1))
        for s, j in zip(sorted(rng.choice(r, size=keep, replace=False).tolist()), ids):
            g0[i, s] = j
    assert ((g0[:, :-1] == INVALID) & (g0[:, 1:] != INVALID)).any()
    idx = vg.Index(ctx, 200, 16, vg.Metric(0))
    idx.set_vectors(base[:200])
    idx.set_vamana_graph(g0, 17)
    idx.insert_vamana(base[200:], r=r, l=20, max_batch=8, growth_div=8)
    graph, entry = ref.insert(base, 200, ref.lists_of(g0), 17, r=r, l=20, max_batch=8, growth_div=8)
    assert ref.STATS["full_prunes"] > 0
    # every list the call wrote is a dense prefix padded with INVALID; a list it did not touch keeps its holes
    g, e = idx.get_vamana_graph()
    eg = ref.array_of(graph, r)
    assert e == entry and g.shape == eg.shape
    kept_holes = rewritten = 0
    for i in range(300):
        if np.array_equal(g[i], eg[i]):
            rewritten += i < 200 and not np.array_equal(g[i], g0[i])
            continue
        assert i < 200 and np.array_equal(g[i], g0[i]) and g[i][g[i] != INVALID].tolist() == graph[i], i
        kept_holes += 1
    assert kept_holes > 0 and rewritten > 0


def test_insert_with_deleted(vg, ctx):  # row 11
    rng = np.random.default_rng(12)
    base = rng.integers(0, 3, (400, 8)).astype(np.float32)
    idx, g0, e0 = _built(vg, ctx, base[:300], 8, 20)
    deleted = rng.random(300) < 0.3
    idx.insert_vamana(base[300:], r=8, l=20, deleted=deleted, max_batch=8, growth_div=8)
    graph, entry = ref.insert(base, 300, ref.lists_of(g0), e0, r=8, l=20, deleted=deleted, max_batch=8, growth_div=8)
    assert ref.STATS["deleted_dropped"] > 0 and ref.STATS["pruned"]  # a full target's reverse-edge prune met deleted ids
    g = _same_graph(idx, graph, entry, 8)
    dead = set(np.nonzero(deleted)[0].tolist())
    for i in list(range(300, 400)) + sorted(ref.STATS["pruned"]):  # the new lists, and the full targets' pruned ones
        assert not dead & set(g[i][g[i] != INVALID].tolist()), i
    # deleted rows are walked through and never returned
    q = base[rng.choice(400, 16, replace=False)]
    alld = np.concatenate([deleted, np.zeros(100, bool)])
    ids, sc, cnt = idx.search_vamana_fresh(q, 10, l=40, deleted=alld)
    eids, esc, ecnt = ref.search(base, graph, entry, q, 10, l=40, deleted=alld)
    assert np.array_equal(cnt, ecnt) and np.array_equal(ids, eids) and np.array_equal(_bits(sc), _bits(esc))
    assert not dead & set(ids[ids != INVALID].tolist())


def test_entry_point_moves_at_500(vg, ctx):  # row 12
    rng = np.random.default_rng(13)
    base = rng.standard_normal((1050, 16)).astype(np.float32)
    assert ref.entry_moves(500, ref.ENTRY_SEED)
    idx = vg.Index(ctx, 0, 16, vg.Metric(0))
    idx.insert_vamana(base[:450], r=12, l=30, seed=ref.ENTRY_SEED, max_batch=1)
    g1, e1 = ref.insert(base[:450], 0, r=12, l=30, seed=ref.ENTRY_SEED, max_batch=1)
    assert idx.get_vamana_graph()[1] == e1 == 98
    idx.insert_vamana(base[450:], r=12, l=30, seed=ref.ENTRY_SEED, max_batch=1)
    g2, e2 = ref.insert(base, 450, g1, e1, r=12, l=30, seed=ref.ENTRY_SEED, max_batch=1)
    assert e2 != 98 and e2 in (499, 999)
    _same_graph(idx, g2, e2, 12)


def test_one_call_equals_two_and_the_index_grows(vg, ctx):  # row 13
    rng = np.random.default_rng(14)
    base = rng.standard_normal((500, 32)).astype(np.float32)
    one = vg.Index(ctx, 0, 32, vg.Metric(0))
    one.insert_vamana(base, r=16, l=40, max_batch=1)
    two = vg.Index(ctx, 0, 32, vg.Metric(0))
    two.insert_vamana(base[:200], r=16, l=40, max_batch=1)
    two.insert_vamana(base[200:], r=16, l=40, max_batch=1)  # 200 -> 500 rows: past 1.5 x the capacity
    g1, e1 = one.get_vamana_graph()
    g2, e2 = two.get_vamana_graph()
    assert g1.shape == g2.shape == (500, 16) and e1 == e2 and np.array_equal(g1, g2)
    graph, entry = ref.insert(base, 0, r=16, l=40, max_batch=1)
    _same_graph(two, graph, entry, 16)
    # the DiskANN walk sees the grown index: the oracle's search over the same graph and rows
    ov = o.VamanaIndex(g2, e2, 32, base=base)
    q = base[rng.choice(500, 8, replace=False)] + np.float32(0.01)
    ids, sc = two.search_vamana(q, 10)
    for qi in range(q.shape[0]):
        eid, esc, _ = ov.search(q[qi], 10)
        assert np.array_equal(ids[qi, :eid.size], eid) and np.array_equal(_bits(sc[qi, :eid.size]), _bits(esc)), qi
    assert ids[ids != INVALID].max() >= 200  # rows of the second call are found


# ---- search parity over a grown graph -----------------------------------------------------------------
@pytest.fixture(scope="module")
def grown(vg, ctx):
    rng = np.random.default_rng(21)
    base = rng.standard_normal((600, 64)).astype(np.float32)
    idx = vg.Index(ctx, 0, 64, vg.Metric(0))
    idx.insert_vamana(base[:400], max_batch=64, growth_div=8)
    idx.insert_vamana(base[400:], max_batch=64, growth_div=8)
    g, e = idx.get_vamana_graph()
    queries = rng.standard_normal((64, 64)).astype(np.float32)
    return idx, base, ref.lists_of(g), e, queries, rng


def _check_search(grown, k, nq=64, deleted=None, mask=None):
    idx, base, graph, entry, queries, _ = grown
    q = queries[:nq]
    ids, sc, cnt = idx.search_vamana_fresh(q, k, deleted=deleted, mask=mask)
    eids, esc, ecnt = ref.search(base, graph, entry, q, k, deleted=deleted, mask=mask)
    assert np.array_equal(cnt, ecnt)
    assert np.array_equal(ids, eids)
    assert np.array_equal(_bits(sc), _bits(esc))
    return ids, cnt


def test_search_k10(grown):
    ids, cnt = _check_search(grown, 10)
    assert (cnt == 10).all()


def test_search_k100(grown):  # ef = 200
    _check_search(grown, 100, nq=16)


def test_search_k1024(grown):  # ef = 2048: the largest the LDS lists serve; the 600-row graph runs dry
    ids, cnt = _check_search(grown, 1024, nq=4)
    assert (cnt <= 600).all() and (ids[:, 600:] == INVALID).all()


def test_search_deleted(grown):
    deleted = grown[5].random(600) < 0.3
    ids, _ = _check_search(grown, 10, nq=32, deleted=deleted)
    assert not deleted[ids[ids != INVALID]].any()


def test_search_shared_mask(grown):  # SearchWithFilter: ef = max(10 k, 2 l)
    mask = grown[5].random(600) < 0.2
    ids, _ = _check_search(grown, 10, nq=32, mask=mask)
    assert mask[ids[ids != INVALID]].all()


def test_search_mask_per_query(grown):
    mask = grown[5].random((16, 600)) < 0.1
    deleted = grown[5].random(600) < 0.2
    ids, cnt = _check_search(grown, 10, nq=16, deleted=deleted, mask=mask)
    for qi in range(16):
        assert mask[qi][ids[qi, :cnt[qi]]].all()


# ---- the reference's recall floor ----------------------------------------------------------------------
@pytest.mark.parametrize("schedule", list(ref.RECALL_SCHEDULES))
def test_recall_floor(vg, ctx, schedule):
    base, queries, graph, entry, eids, esc, ecnt = ref.recall_case(schedule)
    mb, gd = ref.RECALL_SCHEDULES[schedule]
    idx = vg.Index(ctx, 0, 128, vg.Metric(0))
    idx.insert_vamana(base, max_batch=mb, growth_div=gd)
    _same_graph(idx, graph, entry, ref.DEFAULT_R)
    ids, sc, cnt = idx.search_vamana_fresh(queries, 10)
    assert np.array_equal(ids, eids) and np.array_equal(cnt, ecnt) and np.array_equal(_bits(sc), _bits(esc))
    recall = ref.brute_recall(base, queries, ids, 10)
    print(f"recall@10 {schedule}: {recall:.3f}")
    assert recall >= ref.RECALL_FLOOR


# ---- limits ---------------------------------------------------------------------------------------------
def _refused(vg, status, number, call):
    with pytest.raises(vg.VecgoHipError) as e:
        call()
    assert e.value.status == status, e.value
    assert str(number) in e.value.message, e.value.message


def test_limits(vg, ctx):
    rng = np.random.default_rng(30)
    base = rng.standard_normal((64, 16)).astype(np.float32)
    idx = vg.Index(ctx, 0, 16, vg.Metric(0))
    _refused(vg, ERR_UNSUPPORTED, 65, lambda: idx.insert_vamana(base, r=65))
    _refused(vg, ERR_UNSUPPORTED, 1025, lambda: idx.insert_vamana(base, l=1025))
    _refused(vg, ERR_INVALID_ARG, 0, lambda: idx.insert_vamana(base, max_batch=0))
    assert idx.n == 0
    idx.insert_vamana(base, r=8, l=20)
    _refused(vg, ERR_INVALID_ARG, 8, lambda: idx.insert_vamana(base, r=12))
    _refused(vg, ERR_UNSUPPORTED, 2049, lambda: idx.search_vamana_fresh(base[:2], 1, l=2049))
    _refused(vg, ERR_UNSUPPORTED, 2050, lambda: idx.search_vamana_fresh(base[:2], 205, mask=np.ones(64, bool)))
    assert idx.n == 64 and idx.get_vamana_graph()[0].shape == (64, 8)
    bare = vg.Index(ctx, 64, 16, vg.Metric(0))
    bare.set_vectors(base)
    _refused(vg, ERR_NOT_READY, 64, lambda: bare.insert_vamana(base))
    pq = vg.ProductQuantizer(ctx, 16, 4, 256)
    pq.train(np.tile(base, (8, 1)), iters=2, seed=1)
    bare.set_vamana_graph(np.full((64, 8), INVALID, np.uint32), 0)
    bare.set_pq_codes(pq, pq.encode(base))
    _refused(vg, ERR_UNSUPPORTED, "PQ codes", lambda: bare.insert_vamana(base, r=8))
    assert bare.n == 64
    idx.insert_vamana(base[:0], r=8)  # count = 0 changes nothing
    assert idx.n == 64
