"""tests/merge_cases.py without a GPU: every table case reaches the selection path of topk_merge_kernel it was written for
(by the model of the kernel's bounds, merge_path), and the reference the GPU tests compare with — the oracle's CandidateHeap
replayed as the engine's fan-in — is the plain order by (score, global id) wherever that order is defined."""
import numpy as np
import pytest

from tests import merge_cases as mc


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("case", mc.TABLE, ids=lambda c: c.name)
def test_case_reaches_its_path(case, descending):
    ids, sc, off = mc.build(case, descending)
    assert ids.shape == sc.shape == (case.lists, case.nq, case.k) and off.shape == (case.lists,)
    assert ids.dtype == np.uint32 and sc.dtype == np.float32 and off.dtype == np.uint32
    mc.check_path(case, ids, sc, off, descending)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("case", mc.TABLE, ids=lambda c: c.name)
def test_case_is_well_formed(case, descending):
    """best-first lists (as keys: ascending), valid entries a prefix, padding as documented, no NaN, no zero of either sign,
    no (score, global id) twice, every query with scores of its own"""
    ids, sc, off = mc.build(case, descending)
    keys = mc.make_keys(ids, sc, descending, off)
    assert np.all(keys[:, :, 1:] >= keys[:, :, :-1])
    valid = ids != mc.INVALID
    assert np.all(valid[:, :, 1:] <= valid[:, :, :-1])
    assert np.all(sc[~valid] == (-np.inf if descending else np.inf))
    assert not np.isnan(sc).any() and (case.layout == "tied" or not np.any(sc == 0))
    assert np.all(ids[valid] < mc.SPAN)
    for q in range(case.nq):
        kq = keys[:, q][valid[:, q]]
        assert np.unique(kq).size == kq.size
    if case.lists and case.nq > 1:
        assert not np.array_equal(sc[:, 0], sc[:, 1])


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("case", mc.TABLE, ids=lambda c: c.name)
def test_reference_is_the_order_by_score_and_global_id(case, descending):
    ids, sc, off = mc.build(case, descending)
    got_i, got_s, cnt = mc.expected(case, descending)
    k = case.k
    gid = (ids + off[:, None, None]).astype(np.uint32)
    for q in range(case.nq):
        v = ids[:, q] != mc.INVALID
        s, g = sc[:, q][v], gid[:, q][v]
        order = np.lexsort((g, -s if descending else s))[:k]
        r = order.size
        assert cnt[q] == r == min(k, int(v.sum()))
        assert np.array_equal(got_i[q, :r], g[order]), (case.name, q)
        assert np.array_equal(got_s[q, :r].view(np.uint32), s[order].view(np.uint32)), (case.name, q)
        assert np.all(got_i[q, r:] == mc.INVALID) and np.all(got_s[q, r:] == (-np.inf if descending else np.inf))


def test_make_keys_orders_like_the_floats():
    """the model's key is the library's: unsigned order = float order, -0.0 strictly before +0.0, descending reversed"""
    v = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    ids = np.full(v.size, 7, np.uint32)
    up = mc.make_keys(ids, v, False)
    down = mc.make_keys(ids, v, True)
    assert np.all(up[1:] > up[:-1]) and np.all(down[1:] < down[:-1])
    assert mc.make_keys(np.array([mc.INVALID], np.uint32), np.array([1.0], np.float32), False)[0] == mc.KEY_MAX
    off = np.array([5], np.uint32)
    assert mc.make_keys(np.array([[3]], np.uint32), np.array([[1.0]], np.float32), False, off)[0, 0] & np.uint64(0xFFFFFFFF) == 8
