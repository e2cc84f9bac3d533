"""Sequential restatement of vg_vamana_insert and vg_search_vamana_fresh (include/vecgo_hip.h): FreshVamana.Insert
(diskann/fresh_vamana.go:178-222) with searchCandidatesLocked, robustPruneLocked, addReverseEdgeLocked and
maybeUpdateEntryPoint, the batch schedule, the entry-point schedule and `deleted`; FreshVamana.Search / SearchWithFilter
(:272-364) with greedySearch.

Distances are the reference's pair kernels in their summation order (oracle vgo_l2_avx512 / vgo_dot_avx512), cached per
unordered pair of rows: both are symmetric bit for bit.  A list is ordered by (distance, arrival): -0 equals +0, a NaN
orders after +Inf.  Not collected by pytest (no test_ prefix)."""
from __future__ import annotations

import ctypes as C
from bisect import bisect_right

import numpy as np

from oracle import oracle as o
from tests.vamana_build_ref import Pairs

INVALID = 0xFFFFFFFF
ENTRY_PURPOSE = 0x4652455348  # "FRESH": rng_u64(seed, count, ENTRY_PURPOSE, 0)
DEFAULT_R, DEFAULT_L, DEFAULT_ALPHA = 64, 100, 1.2  # FreshDefault* (:20-24)
NAN = float(np.float32(np.nan))
TENTH = float(np.float32(0.1))
# what the last insert() met, for the tests that must reach a path: reverse edges into a full list (and their targets), the
# deleted ids those prunes dropped, and the most reverse edges one target received in one batch
STATS = {"full_prunes": 0, "deleted_dropped": 0, "pruned": set(), "max_records": 0}


def canon(d):
    """The distance as a list keeps it: -0 -> +0, every NaN -> the quiet NaN."""
    d = float(d)
    return NAN if d != d else d + 0.0


def order(d):
    """What a list is sorted by: a NaN after +Inf, NaNs equal among themselves."""
    return (1, 0.0) if d != d else (0, d)


def insert_candidate(keys, items, c, cap):
    """insertCandidate (:898-923) on a list kept as parallel arrays: keys[i] = order(items[i][0]).  The item goes after
    every entry whose distance is <= its own and is dropped when that position is >= cap."""
    w = order(c[0])
    i = bisect_right(keys, w)
    if i >= cap:
        return
    keys.insert(i, w)
    items.insert(i, c)
    if len(keys) > cap:
        keys.pop()
        items.pop()


def walk(dist, graph, entry, ef, is_deleted, skip_deleted):
    """searchCandidatesLocked (:616-671; skip_deleted) / greedySearch (:535-613): dist(id) = the distance of node id to the
    searching vector; returns results as [(distance, id)]."""
    d0 = canon(dist(entry))
    ck, cand = [order(d0)], [(d0, entry)]
    rk, res = [], []
    if not (skip_deleted and is_deleted(entry)):
        rk, res = [order(d0)], [(d0, entry)]
    visited = {entry}
    while cand:
        w = ck.pop(0)
        _, node = cand.pop(0)
        if len(res) >= ef and w > rk[-1]:
            break
        for nb in graph[node]:
            if nb in visited:
                continue
            visited.add(nb)
            c = (canon(dist(nb)), nb)
            insert_candidate(ck, cand, c, 2 * ef)
            if not (skip_deleted and is_deleted(nb)):
                insert_candidate(rk, res, c, ef)
    return res


def prune(dist, node, cands, r, alpha, is_deleted):
    """robustPruneLocked (:748-792) over cands [(distance, id)] in (distance, position) order."""
    a = float(np.float32(alpha))
    sel = []
    for d, c in cands:
        if len(sel) >= r:
            break
        if c == node or is_deleted(c):
            continue
        bound = float(np.float32(a * d))  # the fp32 product: exact in double, rounded once
        if not any(dist(c, s) < bound for s in sel):
            sel.append(c)
    return sel


def add_reverse_edge(dist, graph, target, node, r, alpha, is_deleted):
    """addReverseEdgeLocked (:698-745)."""
    cur = graph[target]
    if node in cur:
        return
    if len(cur) < r:
        graph[target] = cur + [node]
        return
    cands = [(canon(dist(target, c)), c) for c in cur + [node]]
    cands.sort(key=lambda e: order(e[0]))  # stable
    STATS["full_prunes"] += 1
    STATS["pruned"].add(target)
    STATS["deleted_dropped"] += sum(1 for c in cur if is_deleted(c))
    graph[target] = prune(dist, target, cands, r, alpha, is_deleted)


def entry_moves(count, seed):
    """maybeUpdateEntryPoint (:795-801) with the counter RNG in place of rand.Float32()."""
    if count < 100:
        return True
    if count % 500:
        return False
    return (o.rng_u64(seed, count, ENTRY_PURPOSE, 0) >> 40) * 2.0 ** -24 < TENTH


def lists_of(graph_array):
    """[n, r] ids -> lists, empty slots dropped wherever they sit."""
    return [[int(v) for v in row if v != INVALID] for row in np.asarray(graph_array, np.uint32)]


def array_of(graph, r):
    out = np.full((len(graph), r), INVALID, np.uint32)
    for i, lst in enumerate(graph):
        out[i, :len(lst)] = lst
    return out


def insert(base, n_old, graph=None, entry=0, metric=o.METRIC_L2, r=0, l=0, alpha=0.0, deleted=None, seed=0, max_batch=1,
           growth_div=32):
    """Rows n_old .. len(base)-1 of base inserted into `graph` (lists of the first n_old rows; None with n_old = 0).
    deleted: bool[n_old] or None.  Returns (lists of all rows, entry point)."""
    base = np.ascontiguousarray(base, np.float32)
    n_new = base.shape[0]
    r, l, alpha = r or DEFAULT_R, l or DEFAULT_L, alpha or DEFAULT_ALPHA
    dist = Pairs(base, metric)
    dele = None if deleted is None else np.asarray(deleted, bool)
    is_deleted = (lambda i: False) if dele is None else (lambda i: i < dele.size and bool(dele[i]))
    graph = [list(g) for g in (graph or [])] + [[] for _ in range(n_new - n_old)]
    STATS.update(full_prunes=0, deleted_dropped=0, pruned=set(), max_records=0)
    done = n_old
    if n_old == 0 and n_new > 0:
        entry, done = 0, 1
    while done < n_new:
        b = min(max(1, min(done // growth_div, max_batch)), n_new - done)
        snap = list(graph)  # lists are replaced, never changed in place
        new = {}
        for t in range(done, done + b):
            res = walk(lambda i, t=t: dist(i, t), snap, entry, l, is_deleted, True)
            new[t] = prune(dist, t, res, r, alpha, is_deleted)
        for t, lst in new.items():
            graph[t] = list(lst)
        targets = [nb for lst in new.values() for nb in lst]
        STATS["max_records"] = max([STATS["max_records"]] + [targets.count(v) for v in set(targets)])
        for t in range(done, done + b):  # reverse edges: (source, slot) order
            for nb in new[t]:
                add_reverse_edge(dist, graph, nb, t, r, alpha, is_deleted)
        for t in range(done, done + b):
            if entry_moves(t + 1, seed):
                entry = t
        done += b
    return graph, entry


def search(base, graph, entry, queries, k, l=0, metric=o.METRIC_L2, deleted=None, mask=None):
    """vg_search_vamana_fresh: (ids [nq, k], scores, counts).  mask: None, bool[n] or bool[nq, n]."""
    base = np.ascontiguousarray(base, np.float32)
    queries = np.ascontiguousarray(queries, np.float32)
    n, dim = base.shape
    nq = queries.shape[0]
    l = l or DEFAULT_L
    ef = max(2 * k, l) if mask is None else max(10 * k, 2 * l)
    fn = o.lib.vgo_l2_avx512 if metric == o.METRIC_L2 else o.lib.vgo_dot_avx512
    dele = None if deleted is None else np.asarray(deleted, bool)
    is_deleted = (lambda i: False) if dele is None else (lambda i: bool(dele[i]))
    ids = np.full((nq, k), INVALID, np.uint32)
    scores = np.full((nq, k), np.inf if metric == o.METRIC_L2 else -np.inf, np.float32)
    counts = np.zeros(nq, np.int32)
    if n == 0:
        return ids, scores, counts
    p0 = base.ctypes.data
    for qi in range(nq):
        qp = C.cast(queries.ctypes.data + 4 * dim * qi, o._f32p)
        res = walk(lambda i: float(np.float32(fn(C.cast(p0 + 4 * dim * i, o._f32p), qp, dim))), graph, entry, ef,
                   is_deleted, False)
        mk = None if mask is None else (mask if np.ndim(mask) == 1 else mask[qi])
        kept = [(d, i) for d, i in res if not is_deleted(i) and (mk is None or mk[i])][:k]
        counts[qi] = len(kept)
        for j, (d, i) in enumerate(kept):
            ids[qi, j], scores[qi, j] = i, d
    return ids, scores, counts


def brute_recall(base, queries, ids, k):
    """recall@k of ids against exact L2 neighbours (float64 brute force)."""
    b, q = base.astype(np.float64), queries.astype(np.float64)
    d = (q * q).sum(1)[:, None] - 2.0 * q @ b.T + (b * b).sum(1)[None, :]
    truth = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / k for i in range(len(q))]))


# TestFreshVamanaRecall (fresh_vamana_test.go:231-312): 1000 x 128 uniform rows, default options, 50 queries drawn from the
# rows, k = 10, recall >= 0.80.  RECALL_DATA_SEED = 0 clears the floor under both schedules (test_vamana_fresh_cpu.py).
RECALL_DATA_SEED = 0
RECALL_FLOOR = 0.80
RECALL_SCHEDULES = {"serial": (1, 32), "batched": (64, 32)}  # (max_batch, growth_div)
# a seed whose draw at count 500 moves the entry point (entry_moves(500, ENTRY_SEED)); seed 0 moves it at neither 500 nor 1000
ENTRY_SEED = 7
_recall_cache = {}


def recall_case(schedule):
    """(base, queries, lists, entry, ids, scores, counts) of the reference's recall test under a schedule; computed once."""
    if schedule not in _recall_cache:
        rng = np.random.default_rng(RECALL_DATA_SEED)
        base = rng.random((1000, 128), dtype=np.float32)
        queries = base[rng.choice(1000, 50, replace=False)]
        mb, gd = RECALL_SCHEDULES[schedule]
        graph, entry = insert(base, 0, max_batch=mb, growth_div=gd)
        _recall_cache[schedule] = (base, queries, graph, entry) + search(base, graph, entry, queries, 10)
    return _recall_cache[schedule]
