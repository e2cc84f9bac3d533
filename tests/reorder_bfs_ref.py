"""diskann.Writer.reorderBFS (internal/segment/diskann/reorder.go:14-157) restated for the tests of
vg_vamana_reorder_bfs: the order of the writer's queue, and the graph it flushes.

`reorder` is the writer's loop as written: one queue, a visited array, the main BFS from the entry point, then a fresh
BFS from every id still unvisited, in id order.  `reorder_np` is the same order level by level with numpy (a node of
level L+1 goes by the first (parent position, slot) that names it), for large n; the tests check the two agree."""
import numpy as np

INVALID = 0xFFFFFFFF


def _apply(graph, entry, perm, inv):
    g = np.asarray(graph, np.uint32)
    n = g.shape[0]
    rows = g[perm] if n else g
    new_graph = np.where(rows < n, inv[np.minimum(rows, max(n - 1, 0))], rows).astype(np.uint32) if n else rows
    return perm, inv, new_graph, int(inv[entry]) if n else 0


def reorder(graph, entry):
    """(perm, inv_perm, new_graph, new_entry): perm[new] = old, inv_perm[old] = new."""
    g = np.asarray(graph, np.uint32)
    n = g.shape[0]
    perm = []
    inv = np.full(n, INVALID, np.uint32)
    visited = [False] * n
    queue = []
    head = 0

    def drain():
        nonlocal head
        while head < len(queue):
            cur = queue[head]
            head += 1
            inv[cur] = len(perm)
            perm.append(cur)
            for v in g[cur]:
                v = int(v)
                if v == INVALID:  # an empty slot (the reference's lists hold only ids)
                    continue
                if not visited[v]:
                    visited[v] = True
                    queue.append(v)

    if n:
        queue.append(entry)
        visited[entry] = True
        drain()
        for i in range(n):
            if not visited[i]:
                queue.append(i)
                visited[i] = True
                drain()
    assert len(perm) == n
    return _apply(g, entry, np.array(perm, np.uint32), inv)


def reorder_np(graph, entry, stats=None):
    """reorder() level by level; stats (a dict) receives the level count and the number of tail components."""
    g = np.asarray(graph, np.uint32)
    n, r = g.shape
    perm = np.empty(n, np.uint32)
    inv = np.full(n, INVALID, np.uint32)
    placed = 0
    levels = tails = 0

    def bfs(root):
        nonlocal placed, levels
        inv[root] = placed
        perm[placed] = root
        placed += 1
        levels += 1
        level = np.array([root], np.int64)
        while level.size:
            cand = g[level].ravel()  # slot order within parent order = key order
            cand = cand[cand < n]
            cand = cand[inv[cand] == INVALID]
            if not cand.size:
                break
            _, first = np.unique(cand, return_index=True)
            new = cand[np.sort(first)]
            inv[new] = np.arange(placed, placed + new.size, dtype=np.uint32)
            perm[placed:placed + new.size] = new
            placed += new.size
            levels += 1
            level = new.astype(np.int64)

    if n:
        bfs(entry)
        i = 0
        while placed < n:
            rest = np.flatnonzero(inv[i:i + 1024] == INVALID)
            if not rest.size:
                i += 1024
                continue
            i += int(rest[0])
            tails += 1
            bfs(i)
    if stats is not None:
        stats["levels"], stats["tails"] = levels, tails
    return _apply(g, entry, perm, inv)
