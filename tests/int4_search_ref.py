"""What vg_search_int4 must answer, restated for the tests: a row's score is Int4Quantizer.L2Distance (int4.go:136-147, the
precomputed-table order the oracle's l2_distance runs), and the rows that take part are offered in ascending row order to one
searcher.CandidateHeap of capacity k, ReplaceTop at capacity (flat/segment.go:714-721): tests/prefilter_ref.offer_all with
policy="replace_top".  That covers ties (by row id) and NaN scores (the heap's layout decides)."""
import numpy as np

from tests import prefilter_ref

INVALID_ID = 0xFFFFFFFF
QB = 8   # queries a multi-query workgroup carries (kI4sQB, csrc/k_int4_search.hip): the tests' query-block seams


def row_scores(ref, q, codes):
    """float32 [n]: ref.l2_distance(q, code) for every code; ref: oracle.Int4Quantizer with its table"""
    return np.array([ref.l2_distance(q, c) for c in codes], np.float32)


def expected(scores, k, mask=None):
    """(ids [k] uint32, scores [k] float32) over the rows `mask` (bool [n]; None: all) keeps, unused slots INVALID_ID / +Inf"""
    scores = np.asarray(scores, np.float32)
    rows = np.arange(scores.size) if mask is None else np.flatnonzero(np.asarray(mask, np.bool_))
    ids = np.full(k, INVALID_ID, np.uint32)
    sc = np.full(k, np.inf, np.float32)
    if k > 0 and rows.size > 0:
        eid, esc = prefilter_ref.offer_all(rows, scores[rows], k, False, policy="replace_top")
        ids[:eid.size] = eid
        sc[:esc.size] = esc
    return ids, sc


def assert_row(got_ids, got_scores, want_ids, want_scores, what=""):
    """ids exactly, scores by bit pattern, padding slots included.  NaN == NaN: the sign and payload of a NaN are the instruction
    set's (x86 makes 0 * Inf the negative quiet NaN, gfx950 the positive one), not the algorithm's — tests/test_gpu_nonfinite.py's
    rule for every search here."""
    gi = np.asarray(got_ids, np.uint32).reshape(-1)
    gf = np.ascontiguousarray(np.asarray(got_scores, np.float32).reshape(-1))
    wf = np.ascontiguousarray(np.asarray(want_scores, np.float32))
    gs, ws = gf.view(np.uint32), wf.view(np.uint32)
    assert gi.size == want_ids.size, (what, gi.size, want_ids.size)
    bad = np.flatnonzero(gi != want_ids)
    assert bad.size == 0, (what, "ids", bad[:5], gi[bad[:5]], want_ids[bad[:5]])
    bad = np.flatnonzero((gs != ws) & ~(np.isnan(gf) & np.isnan(wf)))
    assert bad.size == 0, (what, "score bits", bad[:5], gs[bad[:5]], ws[bad[:5]])


def spread(nq, extra=3):
    """the queries of a batch a test checks: the first and last query of every block of QB, and a few others"""
    pick = set()
    for q0 in range(0, nq, QB):
        pick.add(q0)
        pick.add(min(q0 + QB, nq) - 1)
    step = max(1, nq // (extra + 1))
    for i in range(1, extra + 1):
        pick.add(min(nq - 1, i * step + (i % 3)))
    return sorted(pick)
