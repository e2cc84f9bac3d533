"""The sequential restatement of the streaming Vamana index (tests/vamana_fresh_ref.py) against the reference's own text
and numbers, on the CPU: insertCandidate as written, the merge the GPU walk performs in its place, the recall floor of
TestFreshVamanaRecall, and the seed the GPU entry-point test uses."""
import numpy as np
import pytest

from tests import vamana_fresh_ref as ref


def go_insert_candidate(slice_, c, max_size):
    """insertCandidate, fresh_vamana.go:898-923, line by line; items are (dist, id)."""
    slice_ = list(slice_)
    lo, hi = 0, len(slice_)  # sort.Search: the first j with slice[j].dist > c.dist
    while lo < hi:
        h = (lo + hi) // 2
        if not slice_[h][0] > c[0]:
            lo = h + 1
        else:
            hi = h
    i = lo
    if i >= max_size:
        return slice_
    if len(slice_) < max_size:
        slice_.append(None)
    if i < len(slice_) - 1:
        slice_[i + 1:] = slice_[i:-1]
    slice_[i] = c
    if len(slice_) > max_size:
        slice_ = slice_[:max_size]
    return slice_


def ref_insert_candidate(items, c, cap):
    keys, items = [ref.order(d) for d, _ in items], list(items)
    ref.insert_candidate(keys, items, c, cap)
    assert keys == [ref.order(d) for d, _ in items]
    return items


HAND = [
    ([], (1.0, 7), 4),                                        # empty
    ([(1.0, 0), (2.0, 1)], (0.5, 7), 4),                      # front
    ([(1.0, 0), (2.0, 1)], (3.0, 7), 4),                      # back, room left
    ([(1.0, 0), (1.0, 1), (2.0, 2)], (1.0, 7), 4),            # a tie goes after its equals
    ([(1.0, 0), (1.0, 1), (1.0, 2), (1.0, 3)], (1.0, 7), 4),  # a full list of ties: position 4 >= cap, dropped
    ([(1.0, 0), (2.0, 1), (3.0, 2), (4.0, 3)], (2.0, 7), 4),  # a full list: the last one falls off
    ([(1.0, 0), (2.0, 1), (3.0, 2), (4.0, 3)], (4.0, 7), 4),  # equal to the last of a full list: dropped
    ([(1.0, 0), (2.0, 1), (3.0, 2), (4.0, 3)], (5.0, 7), 4),  # beyond a full list: dropped
    ([(0.0, 0), (0.0, 1)], (-0.0, 7), 4),                     # -0 equals +0
    ([(1.0, 0)], (0.5, 7), 1),                                # cap 1
]


@pytest.mark.parametrize("items,c,cap", HAND)
def test_insert_candidate_is_the_reference(items, c, cap):
    assert ref_insert_candidate(items, c, cap) == go_insert_candidate(items, c, cap)


def test_insert_candidate_random_with_ties():
    rng = np.random.default_rng(1)
    for _ in range(300):
        cap = int(rng.integers(1, 12))
        a, b = [], []
        for j in range(int(rng.integers(0, 30))):
            c = (float(rng.integers(0, 5)), j)
            a, b = ref_insert_candidate(a, c, cap), go_insert_candidate(b, c, cap)
            assert a == b


def merge_then_cut(pool, fresh, cap):
    """What the GPU walk does per popped node: the fresh entries ordered by (distance, list slot); a pool entry moves up by
    the fresh entries BELOW it, a fresh entry by the pool entries AT OR BELOW it; entries at positions >= cap fall off."""
    fs = sorted(fresh, key=lambda e: ref.order(e[0]))  # stable: list slot breaks ties
    out = {}
    for i, e in enumerate(pool):
        out[i + sum(1 for f in fs if ref.order(f[0]) < ref.order(e[0]))] = e
    for j, f in enumerate(fs):
        out[j + sum(1 for e in pool if ref.order(e[0]) <= ref.order(f[0]))] = f
    assert sorted(out) == list(range(len(pool) + len(fs)))
    return [out[p] for p in range(min(cap, len(out)))]


def test_one_by_one_equals_merge_then_cut():
    rng = np.random.default_rng(2)
    nan = float("nan")
    for trial in range(400):
        cap = int(rng.integers(1, 40))
        values = [0.0, 1.0, 2.0, 3.0, float("inf"), nan] if trial % 4 == 0 else [float(v) for v in range(8)]
        pool = sorted(((values[int(rng.integers(0, len(values)))], 1000 + j) for j in range(int(rng.integers(0, cap + 1)))),
                      key=lambda e: ref.order(e[0]))
        fresh = [(values[int(rng.integers(0, len(values)))], j) for j in range(int(rng.integers(0, 65)))]
        one = list(pool)
        for c in fresh:
            one = ref_insert_candidate(one, c, cap)
        got = merge_then_cut(pool, fresh, cap)
        assert [i for _, i in one] == [i for _, i in got], (trial, cap)


@pytest.mark.parametrize("schedule", list(ref.RECALL_SCHEDULES))
def test_reference_recall_floor(schedule):
    """fresh_vamana_test.go:231-312 on the restatement: default options, k = 10, 50 queries drawn from the rows."""
    base, queries, graph, entry, ids, scores, counts = ref.recall_case(schedule)
    assert (counts == 10).all()
    recall = ref.brute_recall(base, queries, ids, 10)
    print(f"recall@10 {schedule}: {recall:.3f}")
    assert recall >= ref.RECALL_FLOOR
    for i, lst in enumerate(graph):  # structurally valid
        assert len(lst) <= ref.DEFAULT_R and len(set(lst)) == len(lst) and i not in lst and all(0 <= v < 1000 for v in lst)


def test_entry_point_schedule_and_the_recorded_seed():
    assert all(ref.entry_moves(c, 0) for c in range(1, 100))
    assert not any(ref.entry_moves(c, ref.ENTRY_SEED) for c in range(100, 500))
    assert ref.entry_moves(500, ref.ENTRY_SEED)      # the GPU test's seed moves the entry point at count 500
    assert not ref.entry_moves(500, 0) and not ref.entry_moves(1000, 0)
    moved = sum(ref.entry_moves(500 * j, s) for s in range(40) for j in range(1, 26))
    assert 40 < moved < 170  # about one draw in ten of 1000


def test_deleted_rows_are_walked_through_but_never_linked():
    rng = np.random.default_rng(3)
    base = rng.standard_normal((260, 8)).astype(np.float32)
    graph, entry = ref.insert(base[:200], 0, r=6, l=20)
    deleted = rng.random(200) < 0.3
    grown, entry2 = ref.insert(base, 200, graph, entry, r=6, l=20, deleted=deleted)
    dead = set(np.nonzero(deleted)[0].tolist())
    assert ref.STATS["deleted_dropped"] > 0
    for i in list(range(200, 260)) + sorted(ref.STATS["pruned"]):  # the new lists, and the full targets' pruned ones
        assert not dead & set(grown[i]), i
    ids, _, counts = ref.search(base, grown, entry2, base[:20], 5, l=30, deleted=np.concatenate([deleted, np.zeros(60, bool)]))
    assert not dead & set(ids[ids != ref.INVALID].tolist()) and (counts > 0).all()
