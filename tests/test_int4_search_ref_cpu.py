"""tests/int4_search_ref.py against hand-counted cases: it is the yardstick of tests/test_gpu_int4_search.py."""
import numpy as np

from tests import int4_search_ref as ref

INV = ref.INVALID_ID
NAN = float("nan")


def test_ties_go_by_row_id():
    # rows 1, 3, 4 tie at 2.0; row 2 is best; k = 3 keeps 2, then the two lowest tied rows
    ids, sc = ref.expected([5.0, 2.0, 1.0, 2.0, 2.0, 9.0], 3)
    assert ids.tolist() == [2, 1, 3]
    assert sc.tolist() == [1.0, 2.0, 2.0]
    # every row the same score: the k lowest ids, in order, whatever the heap's history
    ids, sc = ref.expected([7.0] * 10, 4)
    assert ids.tolist() == [0, 1, 2, 3] and sc.tolist() == [7.0] * 4


def test_mask_keeps_fewer_than_k_rows():
    mask = np.zeros(8, bool)
    mask[[6, 1]] = True
    ids, sc = ref.expected([0.5, 4.0, 0.1, 0.2, 0.3, 0.4, 3.0, 0.0], 4, mask)
    assert ids.tolist() == [6, 1, INV, INV]
    assert sc[:2].tolist() == [3.0, 4.0] and np.all(np.isposinf(sc[2:]))
    ids, sc = ref.expected([1.0, 2.0], 3, np.zeros(2, bool))    # nothing takes part
    assert ids.tolist() == [INV] * 3 and np.all(np.isposinf(sc))
    ids, sc = ref.expected([3.0, 1.0], 4)                       # fewer rows than k
    assert ids.tolist() == [1, 0, INV, INV]


def test_nan_at_the_root_is_never_replaced():
    # k = 2.  Rows 0, 1 fill the heap: push (NaN, 0), then (5, 1): up() asks Worse((5,1), (NaN,0)) -> scores differ, 5 > NaN is
    # false -> stays below: the root is the NaN.  Every later row is tested against the root: Better(x, (NaN, 0)) -> scores differ,
    # x < NaN false -> rejected.  Pop order: root (NaN, 0) first = worst, then (5, 1): best first is [1, 0].
    ids, sc = ref.expected([NAN, 5.0, 1.0, 0.5], 2)
    assert ids.tolist() == [1, 0]
    assert sc[0] == 5.0 and np.isnan(sc[1])
    # the NaN arrives while the heap is filling but NOT at the root: k = 2, rows (5, 0), (NaN, 1).  up(): Worse((NaN,1), (5,0)) ->
    # NaN > 5 false -> the root stays (5, 0).  Row 2 (1.0) is better than the root: ReplaceTop -> down(): the only child is
    # (NaN, 1); Worse(child, item (1, 2)) -> NaN > 1 false -> the item stays at the root.  Row 3 (0.5) replaces it the same way.
    # Popped: root (0.5, 3), then (NaN, 1): best first [1, 3] — the NaN reports as "best".
    ids, sc = ref.expected([5.0, NAN, 1.0, 0.5], 2)
    assert ids.tolist() == [1, 3]
    assert np.isnan(sc[0]) and sc[1] == 0.5


def test_assert_row_compares_ids_and_score_bits():
    import pytest
    ids = np.array([3, 1, INV], np.uint32)
    sc = np.array([0.0, 2.5, np.inf], np.float32)
    ref.assert_row(ids, sc, ids.copy(), sc.copy())
    with pytest.raises(AssertionError):
        ref.assert_row(np.array([3, 2, INV], np.uint32), sc, ids, sc)
    with pytest.raises(AssertionError):                       # -0.0 and +0.0 are different bits
        ref.assert_row(ids, np.array([-0.0, 2.5, np.inf], np.float32), ids, sc)
    with pytest.raises(AssertionError):                       # a NaN is not a number
        ref.assert_row(ids, np.array([0.0, NAN, np.inf], np.float32), ids, sc)
    with pytest.raises(AssertionError):                       # one slot too few
        ref.assert_row(ids[:2], sc[:2], ids, sc)
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)
    pos_nan = np.array([0x7FC00000], np.uint32).view(np.float32)
    ref.assert_row(ids[:1], neg_nan, ids[:1], pos_nan)        # a NaN's sign is the instruction set's


def test_spread_covers_block_seams():
    qb = ref.QB
    s = ref.spread(2 * qb + 1)
    for q in (0, qb - 1, qb, 2 * qb - 1, 2 * qb):
        assert q in s
    assert ref.spread(1) == [0]
    assert all(0 <= q < 130 for q in ref.spread(130)) and 129 in ref.spread(130)
