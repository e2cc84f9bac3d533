"""The engine's SearchThreshold filter (engine/engine.go:1518-1529) over one query's search output, as the GPU entry points
vg_search_flat_threshold / vg_search_vamana_threshold apply it: in list order, Score <= t for L2 and Score >= t for Dot and
Cosine (both keep the boundary; a NaN threshold or a NaN score keeps nothing), kept rows compacted to the front, the rest
padded with 0xFFFFFFFF / +Inf (L2) or -Inf (Dot, Cosine)."""
import numpy as np

INVALID = 0xFFFFFFFF


def engine_filter(ids, scores, t, desc, max_results):
    """(ids[max_results], scores[max_results], kept) of the rows of (ids, scores) within threshold t, in order"""
    ids = np.asarray(ids, np.uint32)
    scores = np.asarray(scores, np.float32)
    t = np.float32(t)
    with np.errstate(invalid="ignore"):
        keep = (scores >= t) if desc else (scores <= t)
    keep &= ids != INVALID
    out_ids = np.full(max_results, INVALID, np.uint32)
    out_sc = np.full(max_results, -np.inf if desc else np.inf, np.float32)
    kept = int(keep.sum())
    out_ids[:kept] = ids[keep]
    out_sc[:kept] = scores[keep]
    return out_ids, out_sc, kept
