"""Sequential restatement of vg_vamana_build (include/vecgo_hip.h): diskann.Writer.buildGraph
(diskann/writer.go:362-460) with greedySearch, robustPrune and addBackEdge, batches included.

Distances are oracle.l2 / oracle.dot (the reference's pair kernels in their summation order), cached per
unordered pair: both are symmetric bit for bit.  Sorts ascend by the canonical (distance, id) key: -0 equals +0,
every NaN after +Inf, ties by id.  Not collected by pytest (no test_ prefix)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import oracle as o

INVALID = 0xFFFFFFFF
INIT_PURPOSE = 0x56414D414E41  # "VAMANA": rng_u64(seed, node, INIT_PURPOSE, t)
FLT_MAX = float(np.finfo(np.float32).max)


def key(d, i):
    d = float(d)
    return (1, 0.0, i) if d != d else (0, d, i)


class Pairs:
    """distance.Provider(metric)(a, b) of two rows, cached per unordered pair."""

    def __init__(self, base, metric):
        self.base = np.ascontiguousarray(base, np.float32)
        self.dim = self.base.shape[1]
        self.fn = o.lib.vgo_l2_avx512 if metric == o.METRIC_L2 else o.lib.vgo_dot_avx512
        self.p0 = self.base.ctypes.data
        self.cache = {}

    def ptr(self, i):
        return C.cast(self.p0 + 4 * self.dim * i, o._f32p)

    def __call__(self, a, b):
        k = (a, b) if a < b else (b, a)
        d = self.cache.get(k)
        if d is None:
            d = float(np.float32(self.fn(self.ptr(a), self.ptr(b), self.dim)))
            self.cache[k] = d
        return d


def provider(metric):
    return o.l2 if metric == o.METRIC_L2 else o.dot


def centroid_entry(base, metric):
    """writer.go:386-404: float32 sums in row order / float32(n); the first row with dist < minDist."""
    base = np.ascontiguousarray(base, np.float32)
    n, dim = base.shape
    c = np.zeros(dim, np.float32)
    for row in base:
        c = c + row
    c = c / np.float32(n)
    dist = provider(metric)
    best, entry = np.float32(FLT_MAX), 0
    for i in range(n):
        d = dist(base[i], c)
        if d < best:
            best, entry = d, i
    return c, entry


def initial_graph(n, r, seed):
    """node i: j = rng_u64(seed, i, INIT_PURPOSE, t) % n, t = 0, 1, ...; skip i and repeats; min(r, n-1) ids."""
    g = []
    want = min(r, n - 1)
    for i in range(n):
        row, t = [], 0
        while len(row) < want:
            j = o.rng_u64(seed, i, INIT_PURPOSE, t) % n
            t += 1
            if j != i and j not in row:
                row.append(j)
        g.append(tuple(row))
    return g


def prune(dist, node, cands, r, alpha):
    """robustPrune (writer.go:571-625) over the set cands without node."""
    alpha = np.float32(alpha)
    ids = sorted({c for c in cands if c != node}, key=lambda c: key(dist(c, node), c))
    sel = []
    for c in ids:
        if len(sel) >= r:
            break
        dc = np.float32(dist(c, node))
        if all(not (alpha * np.float32(dist(c, s)) < dc) for s in sel):
            sel.append(c)
    return tuple(sel)


def greedy(dist, graph, q, entry, l):
    """greedySearch (writer.go:472-569) for row q over graph."""
    visited = {entry}
    expanded = set()
    pool = [(key(dist(entry, q), entry), entry)]
    while True:
        pool.sort()
        cur = next((i for i, (_, v) in enumerate(pool) if v not in expanded), -1)
        if cur == -1 or (cur >= l and len(pool) > l):
            break
        expanded.add(pool[cur][1])
        nbrs = graph[pool[cur][1]]
        if len(pool) > l + 50:
            pool = pool[:l + 50]
        for nb in nbrs:
            if nb not in visited:
                visited.add(nb)
                pool.append((key(dist(nb, q), nb), nb))
    pool.sort()
    return [v for _, v in pool[:l]]


def build(base, metric=o.METRIC_L2, r=64, l=100, alpha=1.2, init_graph=None, seed=0, max_batch=1, growth_div=32):
    """(graph[n, r] uint32 padded with INVALID, entry point), as vg_vamana_build leaves them."""
    base = np.ascontiguousarray(base, np.float32)
    n = base.shape[0]
    dist = Pairs(base, metric)
    _, entry = centroid_entry(base, metric)
    if init_graph is None:
        graph = initial_graph(n, r, seed)
    else:
        graph = [tuple(int(v) for v in row if v != INVALID) for row in np.asarray(init_graph, np.uint32)]
    processed = 0
    for p in range(2):
        a = 1.0 if p == 0 else alpha
        t0 = 0
        while t0 < n:
            b = min(max(1, min(processed // growth_div, max_batch)), n - t0)
            snap = list(graph)
            new = {i: prune(dist, i, greedy(dist, snap, i, entry, l) + list(snap[i]), r, a) for i in range(t0, t0 + b)}
            for i, lst in new.items():
                graph[i] = lst
            for i in range(t0, t0 + b):  # back edges: (source, slot) order
                for nb in new[i]:
                    lst = graph[nb]
                    if i in lst:
                        continue
                    lst = lst + (i,)
                    if len(lst) > r:
                        lst = prune(dist, nb, lst, r, a)
                    graph[nb] = lst
            t0 += b
            processed += b
    out = np.full((n, r), INVALID, np.uint32)
    for i, lst in enumerate(graph):
        out[i, :len(lst)] = lst
    return out, entry
