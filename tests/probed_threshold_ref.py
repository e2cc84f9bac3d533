"""Engine.SearchThreshold over a flat segment with codes and / or IVF partitions (engine/engine.go:1485-1531 over
flat/segment.go:447-780), composed from the oracle — what vg_search_flat_probed_threshold has to answer:
  1. flat.Segment.Search(q, k = max_results, nprobes, filter): o.FlatSegment.search (the reference's heap, NaN included)
  2. rerank: Segment.Rerank's exact scores (o.rerank_f32), the candidates ordered by (exact score, row id)
  3. the engine's filter (tests/threshold_ref.engine_filter)
and the segments the CPU and GPU tests share (built from numpy and the oracle alone)."""
import numpy as np

from oracle import oracle as o
from tests.threshold_ref import engine_filter

L2, COS, DOT = o.METRIC_L2, o.METRIC_COSINE, o.METRIC_DOT


def candidates(seg, q, max_results, nprobes=0, mask=None, rerank=False):
    """steps 1 and 2 for one query: (ids, scores), best first"""
    ids, sc = seg.search(q, max_results, nprobes, mask)
    if rerank and ids.size:
        sc = o.rerank_f32(seg.base, seg.dim, q, ids, seg.metric)
        order = np.lexsort((ids, -sc if seg.metric != L2 else sc))
        ids, sc = ids[order], sc[order]
    return ids, sc


def expected(seg, q, t, max_results, nprobes=0, mask=None, rerank=False):
    """(ids[max_results], scores[max_results], kept) for one query"""
    ids, sc = candidates(seg, q, max_results, nprobes, mask, rerank)
    return engine_filter(ids, sc, t, seg.metric != L2, max_results)


def rank_threshold(seg, q, rank, max_results, nprobes=0, mask=None, rerank=False):
    """the score of the query's rank-th result ("none": a threshold nothing passes, "all": one everything passes); a rank
    beyond what the query can see is lowered to its last result"""
    desc = seg.metric != L2
    if rank == "none":
        return np.float32(np.inf if desc else -np.inf)
    if rank == "all":
        return np.float32(-np.inf if desc else np.inf)
    _, sc = candidates(seg, q, max_results, nprobes, mask, rerank)
    if sc.size == 0:
        return np.float32(0.0)
    return np.float32(sc[min(rank, sc.size) - 1])


def partitioned(rng, n, dim, parts, metric=L2, empty=(), integer=False, dup=1):
    """Rows grouped by their closest centroid, as flat/writer.go lays a partitioned segment out (unequal sizes, offsets at no
    multiple of anything); the partitions in `empty` get no rows.  integer: small integer values (many equal scores);
    dup: every distinct row that many times."""
    x = rng.standard_normal((n // dup, dim)).astype(np.float32)
    if integer:
        x = np.rint(x * 1.5).astype(np.float32)
    x = np.repeat(x, dup, axis=0)
    cent = (rng.standard_normal((parts, dim)) * 0.7).astype(np.float32)
    a = np.asarray(o.assign_partition_batch(x, cent, metric), np.int64)
    for e in empty:
        a[a == e] = (e + 1) % parts
    order = np.argsort(a, kind="stable")
    x, a = x[order], a[order]
    off = np.searchsorted(a, np.arange(parts + 1)).astype(np.uint32)
    return np.ascontiguousarray(x), cent, off


def sq8_of(x, dim):
    """the oracle's ScalarQuantizer trained on the rows, and their codes"""
    sq = o.ScalarQuantizer(dim)
    sq.train(x)
    return sq, sq.encode_batch(x)


def pq_of(x, dim, m, train_rows=1000, iters=4, seed=2):
    """the oracle's ProductQuantizer (256 centroids) trained on the first rows, and every row's code"""
    pq = o.ProductQuantizer(dim, m, 256)
    pq.train(x[:train_rows], iters=iters, seed=seed)
    return pq, pq.encode_batch(x)
