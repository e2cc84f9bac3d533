"""vg_vamana_build without a GPU: the sequential restatement (tests/vamana_build_ref.py) against the oracle and the
reference's own writer test, and the C ABI's exports."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as o
from tests import vamana_build_ref as ref


@pytest.mark.parametrize("metric", [o.METRIC_L2, o.METRIC_DOT])
def test_restatement_prune_matches_oracle(metric):
    rng = np.random.default_rng(11)
    for case in range(20):
        n, dim = int(rng.integers(8, 80)), int(rng.choice([4, 17, 64]))
        base = rng.standard_normal((n, dim)).astype(np.float32) + 0.5  # no zero distances
        node = int(rng.integers(n))
        cands = rng.choice(n, size=int(rng.integers(1, n)), replace=False).astype(np.uint32)
        r, alpha = int(rng.integers(1, 12)), float(rng.choice([1.0, 1.2, 2.0]))
        want = o.robust_prune(base, dim, node, cands, r, alpha, metric)
        got = ref.prune(ref.Pairs(base, metric), node, [int(c) for c in cands], r, alpha)
        assert list(got) == [int(v) for v in want], case


def test_restatement_reference_writer_case():
    # writer_test.go:20-131 TestWriter: 5 rows of dim 4, R 4, L 10, alpha 1.2
    base = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 1, 0, 0]], np.float32)
    # the writer test checks the graph's size: 5 rows of R = 4 slots.  robustPrune with alpha 1.2 keeps fewer than R
    # where a neighbour is shadowed (row 0 drops row 1: 1.2 * d(1, 4) = 1.2 < d(1, 0) = 2); empty slots pad to R
    g, entry = ref.build(base, o.METRIC_L2, r=4, l=10, alpha=1.2)
    assert g.shape == (5, 4) and 0 <= entry < 5
    for i, row in enumerate(g):
        ids = [int(v) for v in row if v != ref.INVALID]
        assert ids and len(set(ids)) == len(ids) and i not in ids and all(v < 5 for v in ids), (i, row)
        assert all(v == ref.INVALID for v in row[len(ids):]), (i, row)
    assert g[0].tolist() == [4, 2, 3, ref.INVALID]


def test_restatement_initial_graph_follows_rng():
    n, r, seed = 50, 8, 7
    g = ref.initial_graph(n, r, seed)
    for i, row in enumerate(g):
        expect, t = [], 0
        while len(expect) < r:
            j = o.rng_u64(seed, i, ref.INIT_PURPOSE, t) % n
            t += 1
            if j != i and j not in expect:
                expect.append(j)
        assert list(row) == expect
    assert [len(x) for x in ref.initial_graph(5, 8, 1)] == [4] * 5 and ref.initial_graph(1, 8, 1) == [()]


def test_restatement_canonical_order():
    assert ref.key(-0.0, 1) < ref.key(0.0, 2) and ref.key(0.0, 1) < ref.key(-0.0, 2)
    assert ref.key(float("inf"), 9) < ref.key(float("nan"), 0) < ref.key(float("nan"), 1)


def test_abi_exports_and_null_index():
    from vecgo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vg_vamana_build") and hasattr(lib, "vg_index_get_vamana_graph")
    assert lib.vg_abi_minor() >= 12
    assert lib.vg_vamana_build(None, 0, 0, C.c_float(0), None, C.c_uint64(0), 1, 1, None) != 0
    assert lib.vg_index_get_vamana_graph(None, None, None, None, None) != 0
