"""Consolidating the deletes of a resident Vamana graph on the GPU (vg_vamana_consolidate) vs the sequential restatement of
the header's rules (tests/vamana_consolidate_ref.py): the same graph bit for bit, list order and untouched holes included,
the same entry point, the same four counters; then vg_search_vamana_fresh under the same bitmap over the result: the same
ids and score bits.  Then the no-ops, the composition with vg_vamana_insert, device buffers and a caller's stream, and the
refusals.

The split of a batch's visited bitmaps over several launches is tests/test_gpu_vamana_chunks.py's.  Not covered: two
refusals cannot be reached through the public calls and are not tested: a Hamming index takes no fp32 rows ("no fp32 vectors" comes first), and no call installs a graph with r outside
1..64."""
import ctypes as C

import numpy as np
import pytest

from tests import vamana_consolidate_ref as ref
from tests import vamana_fresh_ref as fresh

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
    if kind == "dup":  # every row three times: zero distances, a node's duplicates arrive at distance 0 beside itself
        return np.repeat(rng.standard_normal((n // 3, dim)).astype(np.float32), 3, axis=0)
    if kind == "nan":
        b = rng.standard_normal((n, dim)).astype(np.float32)
        b[n // 3, dim // 2] = np.nan
        return b
    raise ValueError(kind)


def _same_table(idx, want, entry):
    g, e = idx.get_vamana_graph()
    assert g.shape == want.shape
    bad = np.nonzero((g != want).any(1))[0]
    assert bad.size == 0, (bad[:5], g[bad[0]], want[bad[0]])
    assert e == entry
    return g


def _check(idx, base, deleted, metric, l, alpha, max_batch, queries, k=5, expect=None, **call):
    """One consolidate of idx against the restatement run over the graph idx holds; `expect` = the restatement's answer when
    the caller has it already.  Returns (table before, lists after, stats, repaired ids)."""
    g0, e0 = idx.get_vamana_graph()
    r = g0.shape[1]
    graph, stats, repaired = expect or ref.consolidate(base, fresh.lists_of(g0), e0, r, metric=metric, l=l, alpha=alpha,
                                                        deleted=deleted, max_batch=max_batch)
    got = idx.consolidate_vamana(call.pop("deleted_arg", deleted), l=l, alpha=alpha, max_batch=max_batch, **call)
    g1 = _same_table(idx, ref.expected_array(g0, graph, repaired, r), e0)
    assert got == stats, (got, stats)
    assert idx.n == base.shape[0]
    dead = np.nonzero(deleted)[0]
    for i in np.nonzero(~deleted)[0]:  # what the call is for
        assert not np.isin(g1[i], dead).any(), i
    ids, sc, cnt = idx.search_vamana_fresh(queries, k, l=l, deleted=deleted)
    eids, esc, ecnt = fresh.search(base, graph, e0, queries, k, l=l, metric=metric, deleted=deleted)
    assert np.array_equal(cnt, ecnt) and np.array_equal(ids, eids) and np.array_equal(_bits(sc), _bits(esc))
    assert not np.isin(ids[ids != INVALID], dead).any()
    return g0, graph, stats, repaired


# ---- rows 1-3: the schedule case, the restatement computed once (tests/vamana_consolidate_ref.py) ----------------
def _schedule_index(vg, ctx):
    base, deleted, before, entry = ref.schedule_case()
    idx = vg.Index(ctx, 0, 16, vg.Metric(0))
    idx.insert_vamana(base, r=8, l=20, max_batch=1)
    _same_table(idx, fresh.array_of(before, 8), entry)
    return idx, base, deleted


@pytest.mark.parametrize("max_batch", ref.SCHEDULE_BATCHES)
def test_schedule_case(vg, ctx, max_batch):
    idx, base, deleted = _schedule_index(vg, ctx)
    case = ref.schedule_case(max_batch)
    if max_batch != 1:  # the serial loop's graph is another one: max_batch is not ignored
        assert case[4] != ref.schedule_case(1)[4]
    _, _, stats, repaired = _check(idx, base, deleted, 0, 20, 1.2, max_batch, base[::37], expect=case[4:])
    assert stats["repaired_nodes"] == len(repaired) > 32  # more than one batch of 32


# ---- rows 4-11: (n, dim, metric, r, l, alpha, share deleted, max_batch, data, what) -------------------------------
TABLE = [
    (600, 64, 0, 0, 0, 0.0, 0.15, 64, "normal", "defaults"),     # R 64, L 100, alpha 1.2
    (200, 768, 0, 16, 32, 1.2, 0.2, 16, "normal", "dim768"),
    (300, 100, 2, 12, 30, 1.2, 0.2, 16, "normal", "dot"),        # ragged dim, raw Dot ascending
    (300, 100, 1, 12, 30, 1.5, 0.2, 16, "normal", "cosine"),     # Cosine = raw Dot; alpha 1.5
    (400, 8, 0, 8, 20, 1.2, 0.3, 16, "grid", "ties"),            # ties in the lists and in the prune
    (300, 16, 0, 8, 20, 1.2, 0.2, 8, "dup", "dup"),              # zero distances
    (150, 16, 0, 16, 1024, 1.2, 0.2, 8, "normal", "dry"),        # results never fills: the walk runs dry
    (300, 16, 0, 8, 20, 1.2, 0.2, 8, "nan", "nan"),              # a live NaN row
    (300, 16, 0, 8, 20, 1.2, 0.2, 8, "normal", "entry"),         # the entry point is deleted
]


@pytest.mark.parametrize("n,dim,metric,r,l,alpha,share,max_batch,data,what", TABLE, ids=[t[-1] for t in TABLE])
def test_table(vg, ctx, n, dim, metric, r, l, alpha, share, max_batch, data, what):
    rng = np.random.default_rng(n * 31 + dim + metric)
    base = _data(data, n, dim, rng)
    deleted = rng.random(n) < share
    idx = vg.Index(ctx, 0, dim, vg.Metric(metric))
    idx.insert_vamana(base, r=r, l=l, alpha=alpha, max_batch=16, growth_div=8)
    entry = idx.get_vamana_graph()[1]
    deleted[entry] = what == "entry"
    queries = base[rng.choice(n, 8, replace=False)]
    if what == "nan":
        deleted[n // 3] = False
        queries = base[[n // 3, 0, 1]]
    g0, graph, stats, repaired = _check(idx, base, deleted, metric, l, alpha, max_batch, queries)
    assert stats["repaired_nodes"] > max_batch  # several batches
    if what == "ties":
        lists = fresh.lists_of(g0)
        d = fresh.Pairs(base, 0)
        assert any(len({d(i, v) for v in graph[i]}) < len(graph[i]) for i in repaired)  # equal distances inside a new list
        assert lists != graph
    if what == "dup":  # a repaired node's twin sits at distance 0 and is kept first, unless it is deleted
        twins = [i for i in repaired if graph[i] and np.array_equal(base[graph[i][0]], base[i])]
        assert twins
    if what == "dry":
        assert n - int(deleted.sum()) < l  # fewer live rows than results holds
    if what == "nan":
        assert all(len(set(lst)) == len(lst) and i not in lst for i, lst in enumerate(graph))
    if what == "entry":
        assert deleted[entry] and any(entry in lst for lst in fresh.lists_of(g0))


# ---- row 12: an uploaded graph with holes ------------------------------------------------------------------
def test_uploaded_graph_with_holes(vg, ctx):
    rng = np.random.default_rng(12)
    n, r = 200, 8
    base = rng.standard_normal((n, 16)).astype(np.float32)
    deleted = rng.random(n) < 0.2
    entry = 17
    deleted[entry] = False
    live, dead = np.nonzero(~deleted)[0], np.nonzero(deleted)[0]
    g0 = np.full((n, r), INVALID, np.uint32)
    for i in range(n):  # random lists with empty slots in mid-list; some full
        ids = [j for j in rng.choice(n, size=r + 1, replace=False).tolist() if j != i][:r]
        keep = r if i % 4 == 0 else int(rng.integers(0, r + 1))
        for s, j in zip(sorted(rng.choice(r, size=keep, replace=False).tolist()), ids):
            g0[i, s] = j
    a, b, c = (int(v) for v in live[live != entry][[3, 11, 29]])
    g0[a] = [live[0], INVALID, INVALID, dead[0], INVALID, INVALID, INVALID, INVALID]  # its only deleted id sits after a hole
    g0[b] = [live[1], INVALID, live[2], INVALID, INVALID, live[5], INVALID, INVALID]  # holes and no deleted id
    g0[g0 == c] = INVALID                                                             # no list points to c ...
    g0[c] = [INVALID, live[4], dead[1], INVALID, INVALID, INVALID, INVALID, INVALID]  # ... and its list names a deleted id
    idx = vg.Index(ctx, n, 16, vg.Metric(0))
    idx.set_vectors(base)
    idx.set_vamana_graph(g0, entry)
    _, graph, stats, repaired = _check(idx, base, deleted, 0, 20, 1.2, 8, base[rng.choice(n, 8, replace=False)])
    g1 = idx.get_vamana_graph()[0]
    assert a in repaired and c in repaired and b not in repaired
    assert np.array_equal(g1[b], g0[b])
    for i in (a, c):  # written dense
        k = len(graph[i])
        assert (g1[i, :k] != INVALID).all() and (g1[i, k:] == INVALID).all()
    holes = lambda t: ((t[:, :-1] == INVALID) & (t[:, 1:] != INVALID)).any(1)
    kept = [i for i in range(n) if i not in set(repaired)]
    assert holes(g0[kept]).sum() > 10 and np.array_equal(g1[kept], g0[kept])  # untouched lists keep their holes
    assert not holes(g1[repaired]).any()
    assert stats["dropped_links"] > stats["repaired_nodes"]  # some lists named several deleted ids


@pytest.mark.parametrize("r", [1, 3, 5, 33])
def test_degrees_that_are_no_power_of_two(vg, ctx, r):
    """the mark pass gives a node pow2(r) lanes (at least 2): degrees below, between and above the powers the table uses"""
    rng = np.random.default_rng(40 + r)
    n = 130
    base = rng.standard_normal((n, 8)).astype(np.float32)
    deleted = rng.random(n) < 0.25
    g0 = np.full((n, r), INVALID, np.uint32)
    for i in range(n):
        ids = [j for j in rng.choice(n, size=r + 1, replace=False).tolist() if j != i][:r]
        g0[i, :len(ids)] = ids
        g0[i, rng.random(r) < 0.2] = INVALID  # holes
    idx = vg.Index(ctx, n, 8, vg.Metric(0))
    idx.set_vectors(base)
    idx.set_vamana_graph(g0, 0)
    _, _, stats, _ = _check(idx, base, deleted, 0, 16, 1.2, 8, base[::17])
    assert stats["repaired_nodes"] > 8


# ---- rows 13 and 14: the reference's Delete test, and its degenerate ends -----------------------------------
def test_reference_delete_shape(vg, ctx):
    base, deleted, before, entry = ref.delete_test_case()
    idx = vg.Index(ctx, 0, 32, vg.Metric(0))
    idx.insert_vamana(base, max_batch=1)
    _same_table(idx, fresh.array_of(before, fresh.DEFAULT_R), entry)
    _check(idx, base, deleted, 0, 0, 0.0, 1, base[:1], k=10)
    ids, _, cnt = idx.search_vamana_fresh(base[:1], 10, deleted=deleted)
    assert cnt[0] == 10 and ids[0].min() >= 50


@pytest.mark.parametrize("live", [(17, 60), (60,)])
def test_all_but_two_and_all_but_one(vg, ctx, live):
    base, _, before, entry = ref.delete_test_case()
    deleted = np.ones(100, bool)
    deleted[list(live)] = False
    idx = vg.Index(ctx, 100, 32, vg.Metric(0))
    idx.set_vectors(base)
    idx.set_vamana_graph(fresh.array_of(before, fresh.DEFAULT_R), entry)
    _, graph, stats, repaired = _check(idx, base, deleted, 0, 0, 0.0, 1, base[:2], k=3)
    assert repaired == sorted(live)
    if len(live) == 2:
        assert graph[live[0]] == [live[1]] and graph[live[1]] == [live[0]]
    else:
        assert graph[live[0]] == [] and stats["links_after"] == 0


# ---- no-ops, composition, buffers ---------------------------------------------------------------------------
def test_no_ops(vg, ctx):
    idx, base, deleted = _schedule_index(vg, ctx)
    g0, e0 = idx.get_vamana_graph()
    for d in (None, np.zeros(300, bool)):
        assert idx.consolidate_vamana(d, l=20, max_batch=32) == ref.ZERO_STATS
        _same_table(idx, g0, e0)
    first = idx.consolidate_vamana(deleted, l=20, max_batch=32)
    assert first == ref.schedule_case(32)[5]
    g1, _ = idx.get_vamana_graph()
    assert idx.consolidate_vamana(deleted, l=20, max_batch=32) == ref.ZERO_STATS  # a second call with the same bitmap
    _same_table(idx, g1, e0)
    empty = vg.Index(ctx, 0, 16, vg.Metric(0))
    assert empty.consolidate_vamana(None) == ref.ZERO_STATS
    stats = (C.c_int64 * 4)(7, 7, 7, 7)  # n == 0 with a bitmap pointer: VG_OK, stats zeroed
    byte = (C.c_uint8 * 1)(0xFF)
    vg.api.check(empty._lib.vg_vamana_consolidate(empty._h, 0, C.c_float(0), byte, 8, stats, None))
    assert list(stats) == [0, 0, 0, 0]


def test_insert_after_consolidate(vg, ctx):
    """row 2, then 50 more rows under the same bitmap: the two restatements chained"""
    idx, base, deleted = _schedule_index(vg, ctx)
    graph, stats, _ = ref.schedule_case(32)[4:]
    entry = ref.schedule_case()[3]
    assert idx.consolidate_vamana(deleted, l=20, max_batch=32) == stats
    more = np.random.default_rng(5).standard_normal((50, 16)).astype(np.float32)
    idx.insert_vamana(more, r=8, l=20, deleted=deleted, max_batch=8, growth_div=8)
    both = np.concatenate([base, more])
    grown, entry2 = fresh.insert(both, 300, graph, entry, r=8, l=20, deleted=deleted, max_batch=8, growth_div=8)
    g = _same_table(idx, fresh.array_of(grown, 8), entry2)
    alld = np.concatenate([deleted, np.zeros(50, bool)])
    assert not np.isin(g[~alld], np.nonzero(alld)[0]).any()  # the reverse edges' prunes brought no deleted id back
    q = both[::29]
    ids, sc, cnt = idx.search_vamana_fresh(q, 5, l=20, deleted=alld)
    eids, esc, ecnt = fresh.search(both, grown, entry2, q, 5, l=20, deleted=alld)
    assert np.array_equal(cnt, ecnt) and np.array_equal(ids, eids) and np.array_equal(_bits(sc), _bits(esc))


def test_device_bitmap_at_an_odd_offset_on_a_callers_stream(vg, ctx):
    """The bitmap as a device view one byte past an allocation's start, still poison (all ones) when the call is made: its
    producer sits behind a delay on the caller's stream, and the call runs on that stream."""
    import torch
    from tests import devbuf
    idx, base, deleted = _schedule_index(vg, ctx)
    packed = np.packbits(deleted, bitorder="little")
    view = devbuf.offset_like(packed, 1)
    staged = devbuf.whole(packed)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    devbuf.late_inputs(side, [view], [staged])
    _check(idx, base, deleted, 0, 20, 1.2, 32, base[::37], expect=ref.schedule_case(32)[4:], deleted_arg=view, stream=side)
    assert np.array_equal(devbuf.to_host(view), packed)  # read where it lies, never written


# ---- refusals -------------------------------------------------------------------------------------------------
def _refused(vg, status, word, call):
    with pytest.raises(vg.VecgoHipError) as e:
        call()
    assert e.value.status == status and str(word) in e.value.message, (e.value.status, e.value.message)


def test_refusals(vg, ctx):
    base, deleted, before, entry = ref.schedule_case()
    g0 = fresh.array_of(before, 8)
    packed = np.packbits(deleted, bitorder="little")
    stats = (C.c_int64 * 4)(7, 7, 7, 7)

    def raw(idx, l, max_batch, handle=True):
        vg.api.check(idx._lib.vg_vamana_consolidate(idx._h if handle else None, C.c_int32(l), C.c_float(1.2),
                                                    C.c_void_p(packed.ctypes.data), C.c_int32(max_batch), stats, None))

    idx = vg.Index(ctx, 300, 16, vg.Metric(0))
    _refused(vg, ERR_INVALID_ARG, "NULL index", lambda: raw(idx, 20, 8, handle=False))
    _refused(vg, ERR_NOT_READY, "no fp32 vectors", lambda: raw(idx, 20, 8))
    idx.set_vectors(base)
    _refused(vg, ERR_NOT_READY, "no Vamana graph", lambda: raw(idx, 20, 8))
    idx.set_vamana_graph(g0, entry)
    _refused(vg, ERR_UNSUPPORTED, 1024, lambda: raw(idx, 1025, 8))
    _refused(vg, ERR_UNSUPPORTED, 1024, lambda: raw(idx, -1, 8))
    _refused(vg, ERR_UNSUPPORTED, 16384, lambda: raw(idx, 20, 16385))
    _refused(vg, ERR_INVALID_ARG, ">= 1", lambda: raw(idx, 20, 0))
    _refused(vg, ERR_UNSUPPORTED, 1024, lambda: raw(idx, 1025, 0))  # in the header's order: l before max_batch
    assert list(stats) == [7, 7, 7, 7]  # written only on VG_OK
    _same_table(idx, g0, entry)
    # an index that also holds PQ codes is accepted (nothing is appended), and its codes answer as before
    pq = vg.ProductQuantizer(ctx, 16, 4, 256)
    pq.train(np.tile(base, (2, 1)), iters=2, seed=1)
    idx.set_pq_codes(pq, pq.encode(base))
    q = base[::41]
    before_pq = idx.search_pq_adc(q, 5)
    raw(idx, 20, 8)
    assert dict(zip(ref.STAT_NAMES, stats)) == ref.schedule_case(8)[5]
    _same_table(idx, ref.expected_array(g0, *ref.schedule_case(8)[4::2], 8), entry)
    after_pq = idx.search_pq_adc(q, 5)
    assert np.array_equal(before_pq[0], after_pq[0]) and np.array_equal(_bits(before_pq[1]), _bits(after_pq[1]))
