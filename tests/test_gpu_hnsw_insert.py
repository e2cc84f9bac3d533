"""Inserting rows into a resident HNSW graph on the GPU (vg_hnsw_insert) vs the oracle's restatement of hnsw.go's insert
path (oracle/vg_oracle_hnsw_build.c) and vs vg_hnsw_build.  The header's parity contract: vg_hnsw_build over b rows equals
vg_hnsw_build over the first a rows followed by vg_hnsw_insert of rows a..b-1 whenever every call boundary is a batch
boundary of the one-call schedule — for any a when max_batch = 1."""
import numpy as np
import pytest

from oracle import oracle as o

pytestmark = pytest.mark.gpu

VG_ERR_INVALID_ARG, VG_ERR_UNSUPPORTED, VG_ERR_NOT_READY = -1, -5, -9


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def _same_graph(a, b):
    l0a, ua, ea = a
    l0b, ub, eb = b
    assert ea == eb
    assert len(ua) == len(ub)
    assert l0a.shape == l0b.shape
    bad = np.nonzero((l0a != l0b).any(1))[0]
    assert bad.size == 0, (bad[:5], l0a[bad[0]], l0b[bad[0]])
    for (sa, aa), (sb, ab) in zip(ua, ub):
        assert np.array_equal(sa, sb)
        assert np.array_equal(aa, ab)


def _base(kind, n, dim, rng):
    if kind == "uniform":
        return rng.random((n, dim)).astype(np.float32)
    if kind == "grid":
        return rng.integers(0, 3, (n, dim)).astype(np.float32)
    if kind == "dups":
        return rng.standard_normal((n // 3, dim)).astype(np.float32)[rng.integers(0, n // 3, n)]
    base = rng.standard_normal((n, dim)).astype(np.float32)
    if kind == "unit":
        base /= np.linalg.norm(base, axis=1, keepdims=True)
    return base


def _boundaries(n, max_batch, growth_div):
    """batch boundaries of the one-call schedule over n rows: clamp(done / growth_div, 1, max_batch) from done = 1"""
    out, done = [], 1
    while done < n:
        b = min(max(done // growth_div, 1), max_batch, n - done)
        done += b
        out.append(done)
    return out[:-1]


def _same_search(idx, base, dim, graph, metric, m, rng, nq=8):
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    ids, sc = idx.search_hnsw(q, 5, 32)
    oidx = o.HnswIndex(base, dim, *graph, metric=metric, m=m)
    for qi in range(nq):
        eid, esc, _ = oidx.search(q[qi], 5, 32)
        assert np.array_equal(ids[qi, :eid.size], eid)
        assert np.array_equal(sc[qi, :eid.size].view(np.uint32), esc.view(np.uint32))


@pytest.mark.parametrize("n,dim,m,ef,metric,kind", [
    (600, 16, 4, 32, 0, "uniform"),     # M0 = 8: rows prune constantly
    (800, 32, 8, 64, 0, "normal"),
    (500, 768, 32, 300, 0, "normal"),   # BASELINE shape of a row: M = 32, M0 = 64, EF = 300
    (700, 100, 6, 48, 0, "normal"),     # ragged dim, M0 = 12
    (600, 24, 8, 64, 2, "unit"),        # Dot
    (600, 24, 8, 64, 1, "unit"),        # Cosine
    (600, 8, 4, 40, 0, "grid"),         # integer grid: equal distances everywhere (heap-order ties)
    (600, 16, 8, 64, 0, "dups"),        # duplicated rows: zero distances and ties
    (1200, 16, 2, 24, 0, "normal"),     # M = 2: many levels
    (40, 8, 8, 16, 0, "normal"),        # fewer nodes than M0: rows never fill
])
def test_sequential_inserts_match_oracle(vg, ctx, n, dim, m, ef, metric, kind):
    """max_batch = 1 (the reference's Insert loop): an empty index grown by calls of 1, 1, 7, 300 and the rest of the rows
    builds the oracle's graph."""
    rng = np.random.default_rng(n * 11 + dim + m)
    base = _base(kind, n, dim, rng)
    want = o.hnsw_build(base, dim, m=m, ef=ef, metric=metric, max_batch=1)
    idx = vg.Index(ctx, 0, dim, vg.Metric(metric))
    done = 0
    for size in (1, 1, 7, 300, n):
        size = min(size, n - done)
        if size == 0:
            break
        idx.insert_hnsw(base[done:done + size], m=m, ef_construction=ef, max_batch=1)
        done += size
        assert idx.n == done
    assert done == n
    _same_graph(idx.get_hnsw_graph(), want)
    _same_search(idx, base, dim, want, metric, m, rng)


def _moves_entry(n, m, a):
    lv, _, _ = o.hnsw_layout(n, m)
    return lv[a:].max() > lv[:a].max()


@pytest.mark.parametrize("n,dim,m,ef,metric,kind,max_batch,growth_div,moves", [
    (3000, 16, 8, 64, 0, "normal", 64, 16, False),
    (1500, 24, 8, 64, 2, "unit", 64, 16, False),     # Dot
    (1200, 8, 4, 40, 0, "grid", 32, 8, False),       # ties
    (3000, 16, 2, 24, 0, "normal", 256, 16, True),   # M = 2: a new top level created inside the insert
])
def test_batched_insert_matches_oracle(vg, ctx, n, dim, m, ef, metric, kind, max_batch, growth_div, moves):
    rng = np.random.default_rng(n + dim * 3 + m)
    base = _base(kind, n, dim, rng)
    cuts = _boundaries(n, max_batch, growth_div)
    if moves:
        cuts = [a for a in cuts if _moves_entry(n, m, a)]
        assert cuts, "no batch boundary below a new top level"
        a = cuts[len(cuts) // 2]
    else:
        a = min(cuts, key=lambda c: abs(c - n // 2))
    want = o.hnsw_build(base, dim, m=m, ef=ef, metric=metric, max_batch=max_batch, growth_div=growth_div)
    idx = vg.Index(ctx, a, dim, vg.Metric(metric))
    idx.set_vectors(base[:a])
    idx.build_hnsw(m=m, ef_construction=ef, max_batch=max_batch, growth_div=growth_div)
    before = idx.get_hnsw_graph()
    idx.insert_hnsw(base[a:], m=m, ef_construction=ef, max_batch=max_batch, growth_div=growth_div)
    assert idx.n == n
    got = idx.get_hnsw_graph()
    if moves:
        assert got[2] != before[2] and len(got[1]) > len(before[1])
    _same_graph(got, want)
    _same_search(idx, base, dim, want, metric, m, rng)


@pytest.mark.parametrize("edge_distances", [False, True])
@pytest.mark.parametrize("n,dim,m,ef,max_batch,growth_div", [
    (900, 16, 8, 64, 1, 32),       # sequential
    (2000, 32, 8, 64, 64, 16),     # batched
])
def test_insert_into_uploaded_graph(vg, ctx, n, dim, m, ef, max_batch, growth_div, edge_distances):
    """The oracle's graph of base[:a] uploaded with set_hnsw_graph (no build state on the device: every row the insert
    reaches has its state derived), then the rest inserted: the oracle's graph of base."""
    rng = np.random.default_rng(n + m + (7 if edge_distances else 0))
    base = rng.standard_normal((n, dim)).astype(np.float32)
    cuts = _boundaries(n, max_batch, growth_div)
    a = min(cuts, key=lambda c: abs(c - 2 * n // 3))
    l0, upper, ep = o.hnsw_build(base[:a], dim, m=m, ef=ef, max_batch=max_batch, growth_div=growth_div)
    want = o.hnsw_build(base, dim, m=m, ef=ef, max_batch=max_batch, growth_div=growth_div)
    idx = vg.Index(ctx, a, dim)
    idx.set_vectors(base[:a])
    idx.set_hnsw_graph(l0, upper, ep, m=m)
    if edge_distances:
        idx.set_hnsw_edge_distances()
    idx.insert_hnsw(base[a:], m=m, ef_construction=ef, max_batch=max_batch, growth_div=growth_div)
    _same_graph(idx.get_hnsw_graph(), want)
    _same_search(idx, base, dim, want, 0, m, rng)


def test_build_then_insert_equals_build_at_size(vg, ctx):
    """200k x 128, M 16: vg_hnsw_build over everything against vg_hnsw_build + vg_hnsw_insert cut at a batch boundary of
    the default schedule (max_batch 8192, growth_div 32)."""
    n, dim, m, ef = 200_000, 128, 16, 100
    rng = np.random.default_rng(200)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    a = min(_boundaries(n, 8192, 32), key=lambda c: abs(c - 150_000))
    full = vg.Index(ctx, n, dim)
    full.set_vectors(base)
    full.build_hnsw(m=m, ef_construction=ef)
    want = full.get_hnsw_graph()
    full.close()
    idx = vg.Index(ctx, a, dim)
    idx.set_vectors(base[:a])
    idx.build_hnsw(m=m, ef_construction=ef)
    idx.insert_hnsw(base[a:], m=m, ef_construction=ef)
    _same_graph(idx.get_hnsw_graph(), want)


@pytest.mark.parametrize("bf16", [False, True])
def test_every_search_sees_the_new_rows(vg, ctx, bf16):
    n, a, dim, m, ef, k = 2000, 1200, 32, 8, 64, 10
    rng = np.random.default_rng(99 + bf16)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    dead_old = rng.random(a) < 0.1
    dead = np.concatenate([dead_old, np.zeros(n - a, bool)])
    idx = vg.Index(ctx, a, dim)
    idx.set_vectors(base[:a])
    idx.build_hnsw(m=m, ef_construction=ef, max_batch=64, growth_div=16)
    idx.set_hnsw_tombstones(dead_old)
    if bf16:
        idx.enable_bf16_filter(True)
    idx.insert_hnsw(base[a:a + 300], m=m, ef_construction=ef, max_batch=64, growth_div=16)
    idx.insert_hnsw(base[a + 300:], m=m, ef_construction=ef, max_batch=64, growth_div=16)
    q = rng.standard_normal((16, dim)).astype(np.float32)
    q[:4] = base[n - 4:]  # new rows as queries: each must be found
    fids, fsc = idx.search_flat(q, k)
    bids, bsc = idx.search_hnsw_brute(q, k)
    graph = idx.get_hnsw_graph()
    oidx = o.HnswIndex(base, dim, *graph, m=m)
    for qi in range(q.shape[0]):
        eid, esc = o.flat_search_f32(base, dim, q[qi], k)
        assert np.array_equal(fids[qi], eid) and np.array_equal(fsc[qi].view(np.uint32), esc.view(np.uint32))
        eid, esc = oidx.brute_search(q[qi], k)
        assert np.array_equal(bids[qi], eid) and np.array_equal(bsc[qi].view(np.uint32), esc.view(np.uint32))
    mask = rng.random(n) < 0.2
    mask[n - 4:] = True

    def same_predicate(deleted, want_deleted):
        pids, psc = idx.search_hnsw_predicate(q, k, ef, mask, deleted=deleted)
        for qi in range(q.shape[0]):
            eid, esc, _ = oidx.search_predicate(q[qi], k, ef, mask, deleted=want_deleted)
            assert np.array_equal(pids[qi, :eid.size], eid)
            assert np.array_equal(psc[qi, :eid.size].view(np.uint32), esc.view(np.uint32))

    same_predicate(dead, dead)
    same_predicate(None, dead)  # no bitmap given: the index's, grown by the insert
    # the index's tombstones: the old deleted rows stay hidden, every new row is live
    oidx.set_tombstones(dead)
    ids, sc = idx.search_hnsw(q, k, ef)
    for qi in range(q.shape[0]):
        eid, esc, _ = oidx.search(q[qi], k, ef)
        assert np.array_equal(ids[qi, :eid.size], eid)
        assert np.array_equal(sc[qi, :eid.size].view(np.uint32), esc.view(np.uint32))
    assert not dead[ids[ids != 0xFFFFFFFF]].any()
    for qi in range(4):
        assert ids[qi, 0] == n - 4 + qi
    idx.set_hnsw_tombstones(None)
    oidx.set_tombstones(None)
    same_predicate(None, None)


def _refused(vg, fn, status, word):
    with pytest.raises(vg.VecgoHipError) as e:
        fn()
    assert e.value.status == status, e.value
    assert word in e.value.message, e.value.message


def test_refusals_and_edge_cases(vg, ctx):
    n, dim, m, ef = 394, 16, 8, 48  # 394: a batch boundary of the (32, 16) schedule
    rng = np.random.default_rng(5)
    base = rng.standard_normal((n + 50, dim)).astype(np.float32)
    extra = base[n:]
    bare = vg.Index(ctx, n, dim)
    bare.set_vectors(base[:n])
    _refused(vg, lambda: bare.insert_hnsw(extra, m=m, ef_construction=ef), VG_ERR_NOT_READY, "vg_hnsw_build")

    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base[:n])
    idx.build_hnsw(m=m, ef_construction=ef, max_batch=32, growth_div=16)
    q = rng.standard_normal((8, dim)).astype(np.float32)
    graph0 = idx.get_hnsw_graph()
    res0 = idx.search_hnsw(q, 5, 32)

    def unchanged():
        assert idx.n == n
        _same_graph(idx.get_hnsw_graph(), graph0)
        ids, sc = idx.search_hnsw(q, 5, 32)
        assert np.array_equal(ids, res0[0]) and np.array_equal(sc.view(np.uint32), res0[1].view(np.uint32))

    _refused(vg, lambda: idx.insert_hnsw(extra, m=4, ef_construction=ef), VG_ERR_INVALID_ARG, "match")
    _refused(vg, lambda: idx.insert_hnsw(extra, m=40, ef_construction=ef), VG_ERR_UNSUPPORTED, "M=40")
    _refused(vg, lambda: idx.insert_hnsw(extra, m=m, ef_construction=2000), VG_ERR_UNSUPPORTED, "ef_construction")
    _refused(vg, lambda: idx.insert_hnsw(extra, m=m, ef_construction=ef, max_batch=0), VG_ERR_INVALID_ARG, "max_batch")
    unchanged()
    idx.insert_hnsw(np.zeros((0, dim), np.float32), m=m, ef_construction=ef)  # count = 0: a no-op
    unchanged()

    # segment state the appended rows would lack
    idx.set_partitions(rng.standard_normal((2, dim)).astype(np.float32), np.array([0, n // 2, n], np.uint32))
    _refused(vg, lambda: idx.insert_hnsw(extra, m=m, ef_construction=ef), VG_ERR_UNSUPPORTED, "IVF partitions")
    idx.set_partitions(None, [])
    unchanged()
    vam = vg.Index(ctx, n, dim)
    vam.set_vectors(base[:n])
    vam.build_hnsw(m=m, ef_construction=ef)
    vam.set_vamana_graph(np.full((n, 8), 0xFFFFFFFF, np.uint32), 0)
    _refused(vg, lambda: vam.insert_hnsw(extra, m=m, ef_construction=ef), VG_ERR_UNSUPPORTED, "Vamana")
    rq = vg.Index(ctx, n, dim)
    rq.set_vectors(base[:n])
    rq.build_hnsw(m=m, ef_construction=ef)
    cb = int(rq._lib.vg_rabitq_code_bytes(dim))
    rq.set_rabitq_codes(np.zeros(n * cb, np.uint8))
    _refused(vg, lambda: rq.insert_hnsw(extra, m=m, ef_construction=ef), VG_ERR_UNSUPPORTED, "RaBitQ")

    # and the index still takes rows after all of that
    idx.insert_hnsw(extra, m=m, ef_construction=ef, max_batch=32, growth_div=16)
    assert idx.n == n + 50
    assert n in _boundaries(n + 50, 32, 16)
    _same_graph(idx.get_hnsw_graph(), o.hnsw_build(base, dim, m=m, ef=ef, max_batch=32, growth_div=16))
