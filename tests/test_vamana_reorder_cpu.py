"""vg_vamana_reorder_bfs without a GPU: hand-worked cases of the writer's BFS order (tests/reorder_bfs_ref.py), the
level-by-level restatement against the sequential one, the C ABI's export and refusal, and the bindings."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import reorder_bfs_ref as ref

ROOT = Path(__file__).resolve().parents[1]
X = ref.INVALID


def _g(rows, r):
    return np.array([list(row) + [X] * (r - len(row)) for row in rows], np.uint32)


def _both(g, entry):
    a = ref.reorder(g, entry)
    b = ref.reorder_np(g, entry)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3]
    return a


def test_bfs_order_is_first_discovery_not_id_order():
    # the entry lists 9 before 3: the queue holds 9, then 3; 9's child 1 comes before 3's child 2
    g = _g([[9, 3], [], [], [2], [], [], [], [], [], [1]], 2)
    perm, inv, ng, ne = _both(g, 0)
    assert perm[:5].tolist() == [0, 9, 3, 1, 2]
    assert perm[5:].tolist() == [4, 5, 6, 7, 8]  # the tail: singletons in id order
    assert ne == 0 and inv[9] == 1 and inv[3] == 2
    assert ng[0].tolist() == [1, 2] and ng[1].tolist() == [3, X] and ng[2].tolist() == [4, X]


def test_second_component_root_is_smallest_unvisited_id():
    # component {0, 1}; then the tail starts at 2, which reaches 5 before 3 and 4 (5 is listed first)
    g = _g([[1], [0], [5, 3], [], [2], [4]], 2)
    perm, inv, ng, ne = _both(g, 0)
    assert perm.tolist() == [0, 1, 2, 5, 3, 4]
    assert np.array_equal(inv[perm], np.arange(6))


def test_entry_not_zero():
    g = _g([[1], [2], [0], [0]], 1)
    perm, inv, ng, ne = _both(g, 2)
    assert perm.tolist() == [2, 0, 1, 3] and ne == 0 and inv[2] == 0
    assert ng.ravel().tolist() == [1, 2, 0, 1]


def test_holes_self_edges_and_repeats():
    g = np.array([[X, 2, 0, 2, X, 1], [1, X, X, 3, 3, X], [X, X, X, X, X, X], [0, 1, 2, X, 3, X]], np.uint32)
    perm, inv, ng, ne = _both(g, 0)
    assert perm.tolist() == [0, 2, 1, 3]
    # slot order and holes keep their places; ids go through inv_perm
    assert ng[0].tolist() == [X, 1, 0, 1, X, 2]
    assert ng[2].tolist() == [2, X, X, 3, 3, X]


def test_single_node():
    perm, inv, ng, ne = _both(np.array([[X, X]], np.uint32), 0)
    assert perm.tolist() == [0] and inv.tolist() == [0] and ne == 0
    perm, inv, ng, ne = _both(np.array([[0]], np.uint32), 0)  # a self edge
    assert ng.tolist() == [[0]]


@pytest.mark.parametrize("seed", range(6))
def test_numpy_restatement_matches_sequential(seed):
    rng = np.random.default_rng(seed)
    n, r = int(rng.integers(2, 400)), int(rng.integers(1, 9))
    g = rng.integers(0, n, (n, r)).astype(np.uint32)
    g[rng.random((n, r)) < rng.random()] = X
    g[rng.random(n) < 0.2] = X  # whole empty lists
    _both(g, int(rng.integers(n)))


def test_abi_export_declaration_and_null_index():
    from vecgo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vg_vamana_reorder_bfs") and "vg_vamana_reorder_bfs" in _lib.declared_symbols()
    h = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR (\d+)", h).group(1) == "13"
    assert "vg_vamana_reorder_bfs" in h.split("#define VG_ABI_MINOR")[0]  # named in the minor-13 note
    st = lib.vg_vamana_reorder_bfs(None, None, None, None)
    assert st == -1 and b"NULL index" in lib.vg_last_error()


def test_python_binding_shapes():
    # the binding hands the library two n-long uint32 buffers and returns them as they are
    from vecgo_amd import api
    calls = []

    class FakeLib:
        def vg_vamana_reorder_bfs(self, h, perm, inv, stream):
            calls.append((h, perm, inv))
            n = 5
            p = np.ctypeslib.as_array(C.cast(perm, C.POINTER(C.c_uint32)), (n,))
            q = np.ctypeslib.as_array(C.cast(inv, C.POINTER(C.c_uint32)), (n,))
            p[:] = [4, 3, 2, 1, 0]
            q[:] = [4, 3, 2, 1, 0]
            return 0

    idx = object.__new__(api.Index)
    idx._lib, idx._h, idx.n = FakeLib(), C.c_void_p(1), 5
    perm, inv = idx.reorder_vamana_bfs()
    assert len(calls) == 1 and perm.dtype == np.uint32 and inv.dtype == np.uint32
    assert perm.tolist() == [4, 3, 2, 1, 0] and inv.shape == (5,)


def test_cpp_and_go_mirrors_name_the_call():
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert re.search(r"void ReorderVamanaBFS\(uint32_t \*perm, uint32_t \*invPerm\)", hpp)
    assert "vg_vamana_reorder_bfs(h_, perm, invPerm" in hpp
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    assert "func (r *Resident) ReorderVamanaBFS() (perm, invPerm []uint32, err error)" in go
    assert "C.vg_vamana_reorder_bfs(" in go
