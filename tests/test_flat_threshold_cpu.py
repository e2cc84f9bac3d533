"""No-GPU checks of vg_search_flat_threshold (Engine.SearchThreshold over one flat segment, engine/engine.go:1485-1531): the
library exports it, the ABI minor announces it, a NULL index is an argument error, and the reference's own SearchThreshold
case (internal/engine/batch_test.go:47-67) through the oracle + the engine's filter."""
import ctypes as C
import re

import numpy as np

from oracle import oracle as o
from vecgo_amd import _lib


def threshold_filter(ids, scores, threshold, metric):
    """engine.go:1518-1529: Score <= threshold (L2) / Score >= threshold (Dot, Cosine), in the order Search returned"""
    keep = scores <= threshold if metric == o.METRIC_L2 else scores >= threshold
    return ids[keep], scores[keep]


def test_library_exports_search_flat_threshold():
    lib = _lib.load()
    assert hasattr(lib, "vg_search_flat_threshold")
    assert "vg_search_flat_threshold" in _lib.declared_symbols()


def test_abi_minor_announces_it():
    lib = _lib.load()
    minor = int(re.search(r"#define\s+VG_ABI_MINOR\s+(\d+)", _lib.HEADER_PATH.read_text()).group(1))
    assert lib.vg_abi_minor() == minor >= 11


def test_null_index_is_an_argument_error():
    lib = _lib.load()
    q = np.zeros(4, np.float32)
    t = np.zeros(1, np.float32)
    ids = np.zeros(4, np.uint32)
    sc = np.zeros(4, np.float32)
    cnt = np.zeros(1, np.int32)
    st = lib.vg_search_flat_threshold(None, C.c_void_p(q.ctypes.data), C.c_int64(1), C.c_void_p(t.ctypes.data), C.c_int32(4),
                                      None, C.c_int64(0), C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                      C.c_void_p(cnt.ctypes.data), None)
    assert st == -1   # VG_ERR_INVALID_ARG


def test_reference_search_threshold_case_through_the_oracle():
    """batch_test.go:47-67: rows {1,0}, {0,1}, {1,1}, query {1,0} (L2): threshold 0.5 keeps row 0, 1.1 keeps rows 0 and 2"""
    base = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    q = np.array([1, 0], np.float32)
    eid, esc = o.flat_search_f32(base, 2, q, 10)
    ids, sc = threshold_filter(eid, esc, np.float32(0.5), o.METRIC_L2)
    assert ids.tolist() == [0] and sc.tolist() == [0.0]
    ids, sc = threshold_filter(eid, esc, np.float32(1.1), o.METRIC_L2)
    assert ids.tolist() == [0, 2] and sc.tolist() == [0.0, 1.0]
