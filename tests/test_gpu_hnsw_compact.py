"""Compacting a resident HNSW graph on the GPU (vg_hnsw_compact) vs the plain-Python restatement of compact.go
(tests/hnsw_compact_ref.py): the level tables, the entry point and the four counters bit for bit, for max_batch 1 (the
reference with one worker) and 64; then what the compacted index is for — the walks over it equal the oracle's over the
fetched graph, deleted rows never come back, recall does not fall, vg_hnsw_insert goes on — and the no-ops and refusals.

Every graph of the parity cases comes from o.hnsw_build, uploaded with set_hnsw_graph and set_hnsw_edge_distances(): an
uploaded graph's Neighbor.Dist is the pair kernel's distance, which is what the restatement computes."""
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import hnsw_compact_ref as ref

pytestmark = pytest.mark.gpu

VG_ERR_INVALID_ARG, VG_ERR_UNSUPPORTED, VG_ERR_NOT_READY = -1, -5, -9
INVALID = 0xFFFFFFFF

# name: (n, dim, M, ef, metric, rows, tombstone fraction, seed, extra)
CASES = {
    "m4":       (600, 16, 4, 32, 0, "uniform", 0.5, 1, None),      # small M0: constant repair
    "m8":       (800, 32, 8, 64, 0, "normal", 0.5, 2, "entry"),    # the entry point tombstoned
    "dot":      (600, 24, 8, 64, 2, "unit", 0.5, 3, None),
    "cosine":   (600, 24, 8, 64, 1, "unit", 0.5, 4, None),
    "grid":     (600, 8, 4, 40, 0, "grid", 0.5, 5, None),          # integer grid: ties everywhere
    "small_ef": (600, 16, 8, 16, 0, "normal", 0.5, 6, "hood"),     # merged set larger than EF: the bounded push drops items;
                                                                   # a node's whole neighbourhood tombstoned: numToSelect 0
    "m2":       (1200, 16, 2, 24, 0, "normal", 0.5, 7, None),      # many levels: upper-level repairs, M/2 = 1
    "tiny":     (40, 8, 8, 16, 0, "normal", 0.5, 8, None),         # fewer nodes than M0
    "baseline": (500, 768, 32, 300, 0, "normal", 0.5, 9, None),    # BASELINE row shape
    # The lighter fraction.  A list needs repair only when fewer than HALF its capacity is live, and a built graph's layer-0
    # lists hold between M and 2M members, so with 3 in 10 nodes gone few lists qualify whatever the seed (m4: 31 of 414 live
    # nodes, cosine: 24 of 391, the other shapes fewer): the quarter-of-the-live-nodes condition below cannot be met at this
    # fraction and is asked of the 0.5 cases only; these two must still repair something.
    "m4_30":     (600, 16, 4, 32, 0, "uniform", 0.3, 1, None),
    "cosine_30": (600, 24, 8, 64, 1, "unit", 0.3, 4, None),
}


def _rows(kind, n, dim, rng):
    if kind == "uniform":
        return rng.random((n, dim)).astype(np.float32)
    if kind == "grid":
        return rng.integers(0, 3, (n, dim)).astype(np.float32)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    if kind == "unit":
        base /= np.linalg.norm(base, axis=1, keepdims=True)
    return base


@functools.lru_cache(maxsize=None)
def case(name):
    """the rows, the oracle's graph and the seeded tombstones of a case (computed once, shared, never changed)"""
    n, dim, m, ef, metric, kind, frac, seed, extra = CASES[name]
    rng = np.random.default_rng(seed)
    base = _rows(kind, n, dim, rng)
    l0, upper, entry = o.hnsw_build(base, dim, m=m, ef=ef, metric=metric)
    dead = rng.random(n) < frac
    dead[entry] = extra == "entry"
    if extra == "hood":  # the live node with the fullest layer-0 list loses every neighbour: the kept tombstones fill its list
        counts = (l0 != INVALID).sum(1)
        counts[dead] = -1
        v = int(np.argmax(counts))
        dead[l0[v][l0[v] != INVALID]] = True
        dead[entry] = False
    for a in (base, l0, dead, *(x for s in upper for x in s)):
        a.setflags(write=False)
    return dict(n=n, dim=dim, m=m, ef=ef, metric=metric, base=base, l0=l0, upper=upper, entry=entry, dead=dead)


@functools.lru_cache(maxsize=None)
def expected(name, max_batch):
    c = case(name)
    return ref.compact(c["base"], c["dim"], c["l0"], c["upper"], c["entry"], c["dead"], c["m"], ef=c["ef"], max_batch=max_batch,
                       metric=c["metric"])


def input_is_strong(name):
    """Conditions on the inputs, not measurements.  Fraction 0.5: the restatement repairs at least a quarter of the live nodes
    at layer 0 and rewrites a list above layer 0.  M = 2 is the exception to the second: there a list above layer 0 needs
    repair only when BOTH its members are tombstoned (M/2 = 1), the kept tombstones then fill it and numToSelect is 0 — and a
    one-member list exists only on a level of two nodes, where a walk has nobody else to find — so no seed can make the
    restatement rewrite one; the case must send lists above layer 0 through the repair (walk, merge, nothing to select)."""
    c = case(name)
    _, _, _, stats, detail = expected(name, 1)
    live = int((~c["dead"]).sum())
    at_l0 = sum(1 for lv in detail["need"].values() if 0 in lv)
    if CASES[name][6] < 0.5:
        return at_l0 > 0 and stats["repaired_lists"] > 0
    if name == "m2":
        upper = any(level > 0 for lv in detail["need"].values() for level in lv)
    else:
        upper = any(level > 0 for _, level in detail["rewritten"])
    return at_l0 * 4 >= live and stats["repaired_lists"] > 0 and upper


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def upload(vg, ctx, c, tombstones=True):
    idx = vg.Index(ctx, c["n"], c["dim"], vg.Metric(c["metric"]))
    idx.set_vectors(c["base"])
    idx.set_hnsw_graph(c["l0"], c["upper"], c["entry"], m=c["m"])
    idx.set_hnsw_edge_distances()
    if tombstones:
        idx.set_hnsw_tombstones(c["dead"])
    return idx


def same_graph(got, want):
    l0a, ua, ea = got
    l0b, ub, eb = want
    assert ea == eb and len(ua) == len(ub) and l0a.shape == l0b.shape
    bad = np.nonzero((l0a != l0b).any(1))[0]
    assert bad.size == 0, (bad.size, bad[:5], l0a[bad[0]], l0b[bad[0]])
    for level, ((sa, aa), (sb, ab)) in enumerate(zip(ua, ub), 1):
        assert np.array_equal(sa, sb)
        rows = np.nonzero((aa != ab).any(1))[0]
        assert rows.size == 0, (level, rows.size, rows[:5], aa[rows[0]], ab[rows[0]])


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("max_batch", [1, 64])
@pytest.mark.parametrize("name", list(CASES))
def test_compact_matches_restatement(vg, ctx, name, max_batch):
    c = case(name)
    assert input_is_strong(name), "a weak input: too few repairs for the case to mean anything"
    l0, upper, entry, stats, _ = expected(name, max_batch)
    idx = upload(vg, ctx, c)
    got = idx.compact_hnsw(ef_construction=c["ef"], max_batch=max_batch)
    print(name, max_batch, got)
    same_graph(idx.get_hnsw_graph(), (l0, upper, entry))
    assert got == stats
    assert ref.invariants(*idx.get_hnsw_graph()[:2], c["dead"]) == []


def walks_equal_oracle(idx, base, dim, metric, m, dead, rng, nq=6, k=10, ef=48):
    """search_hnsw, search_hnsw_predicate and search_hnsw_brute over the index = the oracle over the fetched graph"""
    graph = idx.get_hnsw_graph()
    oidx = o.HnswIndex(base, dim, *graph, metric=metric, m=m)
    oidx.set_tombstones(dead)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    sel = rng.random((nq, base.shape[0])) < 0.25
    ids, sc = idx.search_hnsw(q, k, ef)
    pids, psc = idx.search_hnsw_predicate(q, k, ef, sel)
    bids, bsc = idx.search_hnsw_brute(q, k, idx.BRUTE_SCAN, ~dead)
    for qi in range(nq):
        for (gi, gs), (eid, esc) in (((ids, sc), oidx.search(q[qi], k, ef)[:2]),
                                     ((pids, psc), oidx.search_predicate(q[qi], k, ef, sel[qi])[:2]),
                                     ((bids, bsc), oidx.brute_search(q[qi], k, o.BRUTE_SCAN, ~dead))):
            assert np.array_equal(gi[qi, :eid.size], eid), qi
            assert np.array_equal(bits(gs[qi, :eid.size]), bits(esc)), qi
            assert (gi[qi, eid.size:] == INVALID).all()
            assert not dead[eid].any()
    return graph


def recall_at_10(idx, c, q, ef):
    live = np.nonzero(~c["dead"])[0]
    ids, _ = idx.search_hnsw(q, 10, ef)
    hit = 0
    for qi in range(q.shape[0]):
        truth, _ = o.flat_search_f32(c["base"][live], c["dim"], q[qi], 10, c["metric"])
        hit += np.intersect1d(live[truth], ids[qi]).size
    return hit / (10.0 * q.shape[0])


@pytest.mark.parametrize("name", ["m4", "dot", "small_ef"])
def test_walks_after_compacting(vg, ctx, name):
    c = case(name)
    assert not c["dead"][c["entry"]]
    idx = upload(vg, ctx, c)
    idx.compact_hnsw(ef_construction=c["ef"], max_batch=64)
    walks_equal_oracle(idx, c["base"], c["dim"], c["metric"], c["m"], c["dead"], np.random.default_rng(11))


def test_recall_does_not_fall(vg, ctx):
    c = case("dot")  # (checked on the restatement first: at ef 16 this graph answers 0.65 under its tombstones, 0.79 compacted)
    q = np.random.default_rng(12).standard_normal((64, c["dim"])).astype(np.float32)
    idx = upload(vg, ctx, c)
    before = recall_at_10(idx, c, q, 16)
    idx.compact_hnsw(ef_construction=c["ef"], max_batch=64)
    after = recall_at_10(idx, c, q, 16)
    print("recall@10 before / after compacting:", before, after)
    assert after >= before


def test_insert_after_compacting(vg, ctx):
    c = case("m8")  # its entry point is tombstoned and emptied: the new rows reach nothing through it, as in the reference
    c2 = case("cosine_30")
    for cc in (c, c2):
        idx = upload(vg, ctx, cc)
        idx.compact_hnsw(ef_construction=cc["ef"], max_batch=64)
        rng = np.random.default_rng(13)
        more = _rows("unit" if cc["metric"] else "normal", 100, cc["dim"], rng)
        idx.insert_hnsw(more, m=cc["m"], ef_construction=cc["ef"], max_batch=8)
        assert idx.n == cc["n"] + 100
        base = np.concatenate([cc["base"], more])
        dead = np.concatenate([cc["dead"], np.zeros(100, np.bool_)])
        if cc is c2:
            walks_equal_oracle(idx, base, cc["dim"], cc["metric"], cc["m"], dead, rng)
        else:  # the graph is still well-formed and the walks still run
            l0, upper, _ = idx.get_hnsw_graph()
            assert l0.shape[0] == base.shape[0]
            idx.search_hnsw(more[:4], 5, 32)


def test_compact_a_graph_the_index_built(vg, ctx):
    """build_hnsw caches the bounded kernel's sums where the reference does, not the pair kernel's distances: no bit parity
    with the restatement, so compact_test.go's invariants and the counters' consistency"""
    rng = np.random.default_rng(21)
    n, dim, m = 3000, 16, 8
    base = rng.standard_normal((n, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    idx.build_hnsw(m=m, ef_construction=64, max_batch=64, growth_div=16)
    l0, upper, entry = idx.get_hnsw_graph()
    dead = rng.random(n) < 0.4
    dead[entry] = False
    idx.set_hnsw_tombstones(dead)
    dead_links = 0
    for owners, rows in [(np.arange(n), l0)] + [(np.nonzero(s != INVALID)[0], a[s[s != INVALID]]) for s, a in upper]:
        live_rows = rows[~dead[owners]]
        valid = live_rows != INVALID
        dead_links += int(dead[live_rows[valid]].sum())
    stats = idx.compact_hnsw(ef_construction=64, max_batch=512)
    print(stats)
    g1 = idx.get_hnsw_graph()
    assert g1[2] == entry
    assert ref.invariants(g1[0], g1[1], dead) == []
    assert stats["cleared_nodes"] == int(dead.sum())
    assert stats["pruned_links"] == dead_links  # a repair keeps every tombstone of the list it rewrites: none added, none lost
    assert stats["repaired_nodes"] > 0 and 0 < stats["repaired_lists"]
    walks_equal_oracle(idx, base, dim, 0, m, dead, rng)
    # a second compact right after the first prunes and clears nothing more
    again = idx.compact_hnsw(ef_construction=64, max_batch=512)
    assert again["pruned_links"] == 0 and again["cleared_nodes"] == 0
    g2 = idx.get_hnsw_graph()
    assert ref.invariants(g2[0], g2[1], dead) == []
    # and vg_hnsw_insert goes on from the cached distances the compaction rewrote
    more = rng.standard_normal((100, dim)).astype(np.float32)
    idx.insert_hnsw(more, m=m, ef_construction=64, max_batch=8)
    walks_equal_oracle(idx, np.concatenate([base, more]), dim, 0, m, np.concatenate([dead, np.zeros(100, np.bool_)]), rng)


def test_no_tombstones_changes_nothing(vg, ctx):
    c = case("m8")
    zero = dict(repaired_nodes=0, repaired_lists=0, pruned_links=0, cleared_nodes=0)
    q = np.random.default_rng(31).standard_normal((4, c["dim"])).astype(np.float32)
    for tomb in (None, np.zeros(c["n"], np.bool_)):
        idx = upload(vg, ctx, c, tombstones=False)
        if tomb is not None:
            idx.set_hnsw_tombstones(tomb)
        before = idx.search_hnsw(q, 5, 32)
        assert idx.compact_hnsw(ef_construction=c["ef"]) == zero
        same_graph(idx.get_hnsw_graph(), (c["l0"], c["upper"], c["entry"]))
        after = idx.search_hnsw(q, 5, 32)
        assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1]))


def _refused(vg, call, status, word):
    with pytest.raises(vg.VecgoHipError) as e:
        call()
    assert e.value.status == status and word in e.value.message, (e.value.status, e.value.message)


def test_refusals(vg, ctx):
    import ctypes as C
    c = case("tiny")
    n, dim = c["n"], c["dim"]
    raw = lambda idx, ef, mb: vg.api.check(idx._lib.vg_hnsw_compact(idx._h, C.c_int32(ef), C.c_int32(mb), None, None))
    # no graph / no rows
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(c["base"])
    _refused(vg, lambda: idx.compact_hnsw(), VG_ERR_NOT_READY, "no HNSW graph")
    idx = vg.Index(ctx, n, dim)
    idx.set_hnsw_graph(c["l0"], c["upper"], c["entry"], m=c["m"])
    _refused(vg, lambda: idx.compact_hnsw(), VG_ERR_NOT_READY, "no fp32 vectors")
    # argument limits (past the wrapper's own checks: the library's)
    idx = upload(vg, ctx, c)
    _refused(vg, lambda: raw(idx, 16, 0), VG_ERR_INVALID_ARG, "max_batch")
    _refused(vg, lambda: raw(idx, 1025, 64), VG_ERR_UNSUPPORTED, "ef_construction")
    # (Hamming is refused too, but no index can get that far: a Hamming index takes no fp32 rows, so "no fp32 vectors" comes first)
    # M0 != 2M
    odd = vg.Index(ctx, n, dim)
    odd.set_vectors(c["base"])
    odd.set_hnsw_graph(np.ascontiguousarray(c["l0"][:, :12]), c["upper"], c["entry"], m=c["m"])
    odd.set_hnsw_tombstones(c["dead"])
    _refused(vg, lambda: odd.compact_hnsw(), VG_ERR_UNSUPPORTED, "M0")
    # segment state: a Vamana graph, PQ codes
    seg = upload(vg, ctx, c)
    seg.set_vamana_graph(np.zeros((n, 4), np.uint32), 0)
    _refused(vg, lambda: seg.compact_hnsw(), VG_ERR_UNSUPPORTED, "Vamana")
    seg = upload(vg, ctx, c)
    pq = vg.ProductQuantizer(ctx, dim, 4, 256)
    pq.train(np.random.default_rng(1).standard_normal((300, dim)).astype(np.float32), iters=2, seed=1)
    seg.set_pq_codes(pq, pq.encode(c["base"]))
    _refused(vg, lambda: seg.compact_hnsw(), VG_ERR_UNSUPPORTED, "PQ codes")
    # every refused index kept its graph
    for i in (idx, seg):
        same_graph(i.get_hnsw_graph(), (c["l0"], c["upper"], c["entry"]))
