"""vg_search_vamana_threshold and the large-k Vamana walk without a GPU: the symbol is exported and declared, the header tells a
binding how to find it, a NULL index is refused, the bindings name it, and the engine's in-order threshold filter
(tests/threshold_ref.py, what the GPU tests hold the entry point to) behaves as specified on oracle output."""
import ctypes as C
import pathlib
import re

import numpy as np

from tests.threshold_ref import INVALID, engine_filter

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_abi_exports_and_null_index():
    from vecgo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vg_search_vamana_threshold")
    h = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert lib.vg_abi_minor() == int(re.search(r"#define VG_ABI_MINOR (\d+)", h).group(1)) >= 13
    q = (C.c_float * 4)()
    t = (C.c_float * 1)()
    st = lib.vg_search_vamana_threshold(None, q, C.c_int64(1), t, 10, 0, None, C.c_int64(0), None, None, None, None, None)
    assert st == -1  # VG_ERR_INVALID_ARG
    assert b"NULL index" in lib.vg_last_error()


def test_header_declares_threshold_and_the_new_limit():
    h = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert "vg_search_vamana_threshold up (dlsym)" in h   # how a binding finds it: the minor is not bumped
    decl = re.search(r"int32_t vg_search_vamana_threshold\(([^)]*)\);", h)
    assert decl is not None
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["vg_index *idx", "const float *queries", "int64_t nq", "const float *thresholds", "int32_t max_results",
                    "int32_t kind", "const uint8_t *mask", "int64_t mask_stride", "uint32_t *ids", "float *scores",
                    "int32_t *counts", "vg_search_stats *stats", "void *stream"]
    assert "k <= 16384" in h


def test_bindings_name_the_entry_point():
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert "ThresholdResult SearchVamanaThreshold(" in hpp and "vg_search_vamana_threshold(h_," in hpp
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    assert "func (r *Resident) SearchVamanaThreshold(" in go and "C.vg_search_vamana_threshold(" in go
    from vecgo_amd import api
    assert callable(api.Index.search_vamana_threshold)


def test_filter_on_oracle_output():
    """the filter over what the oracle's walk returns (a small graph, k = 600 > 512): order kept, boundary kept"""
    from oracle import oracle as o
    from tests import graphs
    rng = np.random.default_rng(3)
    base = rng.standard_normal((700, 8)).astype(np.float32)
    base[100:110] = base[5]                         # tied scores
    g, entry = graphs.build_vamana(base, r=8, seed=1)
    for metric, desc in ((o.METRIC_L2, False), (o.METRIC_DOT, True)):
        ov = o.VamanaIndex(g, entry, 8, o.VAMANA_F32, metric=metric, base=base)
        ids, sc, _ = ov.search(base[5] + np.float32(0.01), 600)
        assert ids.size == 600
        vals, counts = np.unique(sc, return_counts=True)
        assert np.any(counts > 1)
        t = vals[counts > 1][0]
        tie = sc[sc == t]
        fi, fs, kept = engine_filter(ids, sc, t, desc, 600)
        want = (sc >= t) if desc else (sc <= t)
        assert kept == int(want.sum()) and kept >= tie.size   # every tied row at the boundary is kept
        assert np.array_equal(fi[:kept], ids[want]) and np.array_equal(fs[:kept], sc[want])
        assert np.all(fi[kept:] == INVALID) and np.all(fs[kept:] == (-np.inf if desc else np.inf))
        # +Inf / -Inf thresholds keep everything on one side, nothing on the other
        assert engine_filter(ids, sc, np.inf if not desc else -np.inf, desc, 600)[2] == 600
        assert engine_filter(ids, sc, -np.inf if not desc else np.inf, desc, 600)[2] == 0
        # NaN threshold: nothing
        fi, fs, kept = engine_filter(ids, sc, np.nan, desc, 600)
        assert kept == 0 and np.all(fi == INVALID)


def test_filter_nan_scores_and_padding():
    ids = np.array([4, 9, 2, 7, INVALID], np.uint32)
    sc = np.array([1.0, np.nan, 3.0, np.inf, np.inf], np.float32)
    fi, fs, kept = engine_filter(ids, sc, np.inf, False, 6)
    assert kept == 3 and list(fi[:3]) == [4, 2, 7]        # the NaN score is dropped, +Inf kept at an +Inf threshold
    assert list(fi[3:]) == [INVALID] * 3 and np.all(np.isposinf(fs[3:]))
    fi, fs, kept = engine_filter(ids, sc, 3.0, False, 6)
    assert kept == 2 and list(fi[:2]) == [4, 2]           # the boundary kept
    dsc = np.array([5.0, 3.0, np.nan, -np.inf, -np.inf], np.float32)
    fi, fs, kept = engine_filter(ids, dsc, 3.0, True, 5)
    assert kept == 2 and list(fi[:2]) == [4, 9] and np.all(np.isneginf(fs[2:]))
    assert engine_filter(ids, dsc, -np.inf, True, 5)[2] == 3   # NaN and the padding slot dropped, -Inf kept at a -Inf threshold
