"""HNSW.Compact (internal/hnsw/compact.go:16-34) in plain Python over the (l0, upper, entry_point) layout of
get_hnsw_graph — the statement vg_hnsw_compact is compared with, bit for bit.  Test infrastructure.

The three phases as written: repairActiveNodes / reconcileNode (:36-81, :174-233) with checkRepairNeeded (:332-367),
greedyDescent (:235-258), searchLayerPredicateAware (hnsw.go:1406-1557) on the level's own lists under the filter
"id != node", mergeCandidatesWithActiveNeighbors (:260-287) and updateConnectionsForRepair (:289-328);
pruneNodeConnections (:370-401); clearNodeConnections (:404-421).  The queues are the reference's 4-ary heap
(tests/prioq_py.py), distances and selectNeighbors are the oracle's.  The rules the reference leaves open are
vg_hnsw_compact's (include/vecgo_hip.h): the merged set is pushed back in ascending id order; the nodes to repair are fixed
up front and go in id order in batches of max_batch, each batch over the graph as it stood when the batch began
(max_batch = 1: the reference with one worker); levels that need no repair are skipped (the reference walks them without
effect).  Neighbor.Dist of every slot is the pair kernel's distance: the rule for an uploaded graph whose layer-0 edge
distances were computed from the rows."""
import numpy as np

from oracle import oracle as o
from tests.prioq_py import PrioQ

INVALID = 0xFFFFFFFF


class _Graph:
    def __init__(self, base, dim, l0, upper, metric):
        self.base = np.ascontiguousarray(base, np.float32).reshape(-1, dim)
        self.dim, self.metric = dim, metric
        self.n = self.base.shape[0]
        self.l0 = np.array(l0, np.uint32)
        self.upper = [(np.array(s, np.uint32), np.array(a, np.uint32)) for s, a in upper]
        self._rows = {}
        # Neighbor.Dist per slot, 0 for an empty slot
        self.d0 = self._edge(self.l0, np.arange(self.n))
        self.du = []
        for slot, adj in self.upper:
            owner = np.zeros(adj.shape[0], np.int64)
            have = np.nonzero(slot != INVALID)[0]
            owner[slot[have]] = have
            self.du.append(self._edge(adj, owner))

    def dist_row(self, a):
        """ComputeDistance(id, vec(a)) for every id (vectorstore/columnar.go:29-49), cached"""
        r = self._rows.get(a)
        if r is None:
            every = np.arange(self.n, dtype=np.uint32)  # rerank_f32: the single-pair kernels (l2 / dot), one call per row
            if self.metric == o.METRIC_DOT:
                r = -o.rerank_f32(self.base, self.dim, self.base[a], every, o.METRIC_DOT)
            else:
                r = o.rerank_f32(self.base, self.dim, self.base[a], every, o.METRIC_L2)
                if self.metric == o.METRIC_COSINE:
                    r = np.float32(0.5) * r
            self._rows[a] = r = r.astype(np.float32)
        return r

    def _edge(self, table, owner):
        d = np.zeros(table.shape, np.float32)
        for r in range(table.shape[0]):
            ids = table[r]
            cnt = int(np.argmax(ids == INVALID)) if (ids == INVALID).any() else ids.size
            if cnt:
                d[r, :cnt] = self.dist_row(int(owner[r]))[ids[:cnt]]
        return d

    def level_of(self, node):
        lvl = 0
        for l, (slot, _) in enumerate(self.upper):
            if slot[node] != INVALID:
                lvl = l + 1
        return lvl

    def lists(self, node, level):
        """(ids row, distance row) views, or None when the node has no row on the level"""
        if level == 0:
            return self.l0[node], self.d0[node]
        slot, adj = self.upper[level - 1]
        if slot[node] == INVALID:
            return None
        return adj[slot[node]], self.du[level - 1][slot[node]]


def _members(ids):
    out = []
    for v in ids:
        if v == INVALID:
            break
        out.append(int(v))
    return out


def _search_layer(g, dead, drow, node, ep, ep_d, level, ef):
    """searchLayerPredicateAware (hnsw.go:1406-1557), filter id != node; returns the results queue"""
    visited = np.zeros(g.n, np.bool_)
    visited[ep] = True
    cand, res = PrioQ(False), PrioQ(True)
    cand.push(ep, ep_d)
    if ep != node and not dead[ep]:
        res.push(ep, ep_d)
    misses = 0
    while len(cand):
        cn, cd = cand.pop()
        if len(res) >= ef and cd > res.top()[1]:
            break
        row = g.lists(cn, level)
        if row is None:
            continue
        ids, ds = row
        for i, nid in enumerate(_members(ids)):
            if visited[nid]:
                continue
            visited[nid] = True
            passes, is_del = nid != node, bool(dead[nid])
            misses = 0 if passes else misses + 1
            if passes and not is_del:
                nd = drow[nid]
            elif len(res) < ef // 2:
                nd = ds[i] if ds[i] > 0 else drow[nid]
            elif len(res) < ef:
                if misses > 10:
                    continue
                if ds[i] > 0 and len(res) > 0 and ds[i] > np.float32(res.top()[1] * np.float32(1.5)):
                    continue
                nd = drow[nid]
            else:
                continue
            if len(res) >= ef and nd > res.top()[1]:
                continue
            cand.push(nid, nd)
            if passes and not is_del:
                res.push_bounded(nid, nd, ef)
    return res


def _repair_list(g, dead, node, level, ep, ep_d, ef, m):
    """one (node, level): the new (ids, dists) list, or None when nothing was selected (compact.go:315)"""
    drow = g.dist_row(node)
    res = _search_layer(g, dead, drow, node, ep, ep_d, level, ef)
    uniq = {}
    while len(res):
        nid, d = res.pop()
        uniq[nid] = d
    ids, ds = g.lists(node, level)
    kept = []
    for i, nid in enumerate(_members(ids)):
        if dead[nid]:
            kept.append((nid, ds[i]))
        elif nid not in uniq or ds[i] < uniq[nid]:
            uniq[nid] = ds[i]
    heap = PrioQ(True)
    for nid in sorted(uniq):
        heap.push_bounded(nid, uniq[nid], ef)
    limit = 2 * m if level == 0 else m
    want = max(limit - len(kept), 0)
    drained = []
    while len(heap):
        drained.append(heap.pop())
    drained.reverse()
    if want == 0 or not drained:
        return None
    by_id = dict(drained)
    sel = o.hnsw_select_neighbors(g.base, g.dim, [x[0] for x in drained], [x[1] for x in drained], want, g.metric)
    if len(sel) == 0:
        return None
    return kept + [(int(s), by_id[int(s)]) for s in sel]


def compact(base, dim, l0, upper, entry_point, deleted, m, ef=300, max_batch=1, metric=o.METRIC_L2):
    """-> (l0, upper, entry_point, stats, detail).  stats: vg_hnsw_compact_stats as a dict.  detail: `need` = {node: set of
    levels below their threshold}, `rewritten` = [(node, level)] lists the repair phase rewrote."""
    g = _Graph(base, dim, l0, upper, metric)
    dead = np.asarray(deleted, np.bool_).reshape(g.n)
    stats = dict(repaired_nodes=0, repaired_lists=0, pruned_links=0, cleared_nodes=0)
    detail = dict(need={}, rewritten=[])
    if not dead.any():
        return g.l0, g.upper, entry_point, stats, detail
    top = len(g.upper)
    levels = [g.level_of(v) for v in range(g.n)]

    # checkRepairNeeded for every live node, up front
    for v in range(g.n):
        if dead[v]:
            continue
        for l in range(levels[v] + 1):
            active = sum(1 for x in _members(g.lists(v, l)[0]) if not dead[x])
            if active < (m if l == 0 else m // 2):
                detail["need"].setdefault(v, set()).add(l)
    todo = sorted(detail["need"])
    stats["repaired_nodes"] = len(todo)

    for b0 in range(0, len(todo), max_batch):
        staged = []
        for v in todo[b0:b0 + max_batch]:
            drow = g.dist_row(v)
            cur, cur_d = entry_point, drow[entry_point]  # greedyDescent
            for level in range(top, levels[v], -1):
                changed = True
                while changed:
                    changed = False
                    row = g.lists(cur, level)
                    if row is None:
                        break
                    for nid in _members(row[0]):
                        if drow[nid] < cur_d:
                            cur, cur_d, changed = nid, drow[nid], True
            for level in range(levels[v], -1, -1):
                if level in detail["need"][v]:
                    new = _repair_list(g, dead, v, level, cur, cur_d, ef, m)
                    if new is not None:
                        staged.append((v, level, new))
        for v, level, new in staged:
            ids, ds = g.lists(v, level)
            ids[:] = INVALID
            ds[:] = 0
            ids[:len(new)] = [x[0] for x in new]
            ds[:len(new)] = [x[1] for x in new]
            detail["rewritten"].append((v, level))
    stats["repaired_lists"] = len(detail["rewritten"])

    for v in range(g.n):
        if dead[v]:  # clearNodeConnections
            held = False
            for l in range(levels[v] + 1):
                ids, ds = g.lists(v, l)
                held |= bool((ids != INVALID).any())
                ids[:] = INVALID
                ds[:] = 0
            stats["cleared_nodes"] += int(held)
            continue
        for l in range(levels[v] + 1):  # pruneNodeConnections
            ids, ds = g.lists(v, l)
            mem = _members(ids)
            keep = [i for i, x in enumerate(mem) if not dead[x]]
            if len(keep) == len(mem):
                continue
            stats["pruned_links"] += len(mem) - len(keep)
            kid, kd = ids[keep].copy(), ds[keep].copy()
            ids[:] = INVALID
            ds[:] = 0
            ids[:len(keep)] = kid
            ds[:len(keep)] = kd
    return g.l0, g.upper, entry_point, stats, detail


def invariants(l0, upper, deleted):
    """compact_test.go's checks over a compacted graph: returns a list of violations (empty = fine)"""
    dead = np.asarray(deleted, np.bool_)
    bad = []
    tables = [(0, np.arange(l0.shape[0]), l0)]
    for l, (slot, adj) in enumerate(upper):
        have = np.nonzero(slot != INVALID)[0]
        tables.append((l + 1, have, adj[slot[have]]))
    for level, owners, rows in tables:
        for v, ids in zip(owners, rows):
            mem = _members(ids)
            if (ids[len(mem):] != INVALID).any():
                bad.append(("hole", level, int(v)))
            if dead[v] and mem:
                bad.append(("dead node keeps links", level, int(v)))
            if not dead[v] and any(dead[x] for x in mem):
                bad.append(("live node links to a dead one", level, int(v)))
            if len(set(mem)) != len(mem) or int(v) in mem:
                bad.append(("duplicate or self link", level, int(v)))
    return bad
