"""The engine's bitmap strategy for ONE segment, restated (internal/engine/search.go:602-736): the rows a filter keeps, in
ascending order, each scored with distance.SquaredL2 / distance.Dot and offered to one searcher.CandidateHeap of capacity k —
at capacity `Heap.Pop(); Heap.Push(c)` (search.go:725-733), not ReplaceTop as flat/segment.go:719 does.  The heap is
candidate_queue.go:70-179 with float32 comparisons: what decides the answer once a score is a NaN."""
import numpy as np

from oracle import oracle as o

INVALID_ID = 0xFFFFFFFF


def _better(a, b, desc):
    """InternalCandidateBetter (candidate_queue.go:12-23) within one segment; a, b = (score, row)"""
    if a[0] != b[0]:
        return a[0] > b[0] if desc else a[0] < b[0]
    return a[1] < b[1]


def _worse(a, b, desc):
    """InternalCandidateWorse (:27-38)"""
    if a[0] != b[0]:
        return a[0] < b[0] if desc else a[0] > b[0]
    return a[1] > b[1]


class CandidateHeap:
    """the 4-ary heap, worst candidate at the root (candidate_queue.go:70-179)"""

    def __init__(self, descending):
        self.c = []
        self.desc = bool(descending)

    def __len__(self):
        return len(self.c)

    def push(self, x):          # :70-73
        self.c.append(x)
        self._up(len(self.c) - 1)

    def pop(self):              # :75-82
        n = len(self.c) - 1
        self.c[0], self.c[n] = self.c[n], self.c[0]
        self._down(0, n)
        return self.c.pop()

    def peek(self):             # :86-88
        return self.c[0]

    def replace_top(self, x):   # :100-103
        self.c[0] = x
        self._down(0, len(self.c))

    def _up(self, j):           # :136-147
        item = self.c[j]
        while j > 0:
            i = (j - 1) // 4
            if not _worse(item, self.c[i], self.desc):
                break
            self.c[j] = self.c[i]
            j = i
        self.c[j] = item

    def _down(self, i, n):      # :151-179
        item = self.c[i]
        while True:
            first = 4 * i + 1
            if first >= n:
                break
            best = first
            for c in range(first + 1, min(first + 4, n)):
                if _worse(self.c[c], self.c[best], self.desc):
                    best = c
            if not _worse(self.c[best], item, self.desc):
                break
            self.c[i] = self.c[best]
            i = best
        self.c[i] = item


def scores_of(x, q, rows, metric):
    """float32 score of every listed row: distance.SquaredL2 (L2) or distance.Dot (Dot, Cosine), search.go:606-611"""
    f = o.l2 if metric == o.METRIC_L2 else o.dot
    return np.array([f(q, x[r]) for r in rows], np.float32)


def offer_all(rows, scores, k, desc, policy="pop_push"):
    """search.go:717-733 over (row, score) pairs in order; `policy` at capacity: "pop_push" (the engine's) or "replace_top"
    (flat/segment.go:714-721).  Returns (ids, scores) best first: the heap popped until empty, reversed."""
    h = CandidateHeap(desc)
    for r, s in zip(rows, scores):
        c = (float(np.float32(s)), int(r))
        if len(h) < k:
            h.push(c)
        elif _better(c, h.peek(), desc):
            if policy == "pop_push":
                h.pop()
                h.push(c)
            else:
                h.replace_top(c)
    out = []
    while len(h):
        out.append(h.pop())
    out.reverse()
    return np.array([c[1] for c in out], np.uint32), np.array([c[0] for c in out], np.float32)


def search(x, dim, metric, q, k, mask, policy="pop_push"):
    """one query over one segment: x [n, dim] fp32 rows, mask bool[n]"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, dim)
    q = np.ascontiguousarray(q, np.float32)
    rows = np.flatnonzero(np.asarray(mask, np.bool_))
    if k == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32)
    return offer_all(rows, scores_of(x, q, rows, metric), k, metric != o.METRIC_L2, policy)
