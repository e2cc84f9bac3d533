"""Sequential restatement of vg_vamana_consolidate (include/vecgo_hip.h): FreshVamana.consolidate (diskann/fresh_vamana.go:
803-867) with the batch schedule.  The walk, the prune and the pair distances are tests/vamana_fresh_ref.py's, unchanged.

The nodes to repair are the live nodes that list a deleted id, fixed before the first repair, in ascending id order; per
batch of max_batch of them every node walks the graph as it stood when the batch began (for its own row, from the entry
point, deleted nodes walked through and left out of results), prunes the results, and then the batch's lists are written.
No reverse edges; the entry point stays.  Not collected by pytest (no test_ prefix)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as o
from tests import vamana_fresh_ref as fresh
from tests.vamana_build_ref import Pairs

INVALID = fresh.INVALID
STAT_NAMES = ("repaired_nodes", "dropped_links", "links_before", "links_after")
ZERO_STATS = dict.fromkeys(STAT_NAMES, 0)

# The schedule case (tests/test_vamana_consolidate_cpu.py, rows 1-3 of the GPU table): 300 x 16 normal rows inserted from
# empty with r 8, l 20 and the serial schedule, about 20 % deleted.  With SCHEDULE_DATA_SEED = 316 the graphs after
# max_batch 1, 32 and 16384 differ pairwise (the CPU test asserts it), so an implementation that ignores max_batch cannot
# pass all three.
SCHEDULE_DATA_SEED = 316
SCHEDULE_BATCHES = (1, 32, 16384)
_schedule_cache = {}


def consolidate(base, graph, entry, r, metric=o.METRIC_L2, l=0, alpha=0.0, deleted=None, max_batch=1):
    """graph: lists of ids (empty slots already dropped, an id listed twice kept twice: fresh.lists_of); deleted: bool[n] or
    None.  Returns (lists of all rows, stats dict, the repaired ids in order).  A list that is not repaired is returned as
    it came."""
    base = np.ascontiguousarray(base, np.float32)
    l, alpha = l or fresh.DEFAULT_L, alpha or fresh.DEFAULT_ALPHA
    graph = [list(g) for g in graph]
    if deleted is None or not len(graph):
        return graph, dict(ZERO_STATS), []
    dele = np.asarray(deleted, bool)
    is_deleted = lambda i: bool(dele[i])
    dist = Pairs(base, metric)
    repair = [i for i, lst in enumerate(graph) if not dele[i] and any(dele[v] for v in lst)]
    stats = dict(ZERO_STATS, repaired_nodes=len(repair), dropped_links=sum(int(dele[v]) for i in repair for v in graph[i]),
                 links_before=sum(len(graph[i]) for i in repair))
    for b0 in range(0, len(repair), max_batch):
        snap = list(graph)  # lists are replaced, never changed in place
        new = {}
        for i in repair[b0:b0 + max_batch]:
            res = fresh.walk(lambda j, i=i: dist(j, i), snap, entry, l, is_deleted, True)
            new[i] = fresh.prune(dist, i, res, r, alpha, is_deleted)
        for i, lst in new.items():
            graph[i] = list(lst)
    stats["links_after"] = sum(len(graph[i]) for i in repair)
    return graph, stats, repair


def expected_array(before, graph, repaired, r):
    """The [n, r] table the call leaves: `before` (the table as it stood, holes included) with the repaired rows replaced
    by their new lists as dense prefixes."""
    out = np.array(before, np.uint32, copy=True)
    for i in repaired:
        out[i] = INVALID
        out[i, :len(graph[i])] = graph[i]
    return out


def schedule_case(max_batch=None):
    """(base, deleted, lists before, entry) of the schedule case, and with max_batch the consolidate's (lists, stats,
    repaired) appended; computed once."""
    if "input" not in _schedule_cache:
        rng = np.random.default_rng(SCHEDULE_DATA_SEED)
        base = rng.standard_normal((300, 16)).astype(np.float32)
        deleted = rng.random(300) < 0.2
        graph, entry = fresh.insert(base, 0, r=8, l=20)
        _schedule_cache["input"] = (base, deleted, graph, entry)
    inp = _schedule_cache["input"]
    if max_batch is None:
        return inp
    if max_batch not in _schedule_cache:
        base, deleted, graph, entry = inp
        _schedule_cache[max_batch] = consolidate(base, graph, entry, 8, l=20, deleted=deleted, max_batch=max_batch)
    return inp + _schedule_cache[max_batch]


def delete_test_case():
    """TestFreshVamanaDelete (fresh_vamana_test.go:71-116): 100 x 32 uniform rows inserted with the default options, ids
    0..49 deleted.  (base, deleted, lists before, entry); computed once."""
    if "delete" not in _schedule_cache:
        rng = np.random.default_rng(71)
        base = rng.random((100, 32), dtype=np.float32)
        deleted = np.arange(100) < 50
        graph, entry = fresh.insert(base, 0)
        _schedule_cache["delete"] = (base, deleted, graph, entry)
    return _schedule_cache["delete"]
