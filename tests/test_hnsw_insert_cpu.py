"""vg_hnsw_insert without a GPU: the symbol is exported and declared, the minor version announces it, a NULL index is
refused, and the C++ and Go mirrors name the entry point."""
import ctypes as C
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_abi_exports_and_null_index():
    from vecgo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vg_hnsw_insert")
    assert lib.vg_abi_minor() >= 13
    rows = (C.c_float * 4)()
    st = lib.vg_hnsw_insert(None, rows, C.c_int64(1), 32, 300, 8192, 32, None)
    assert st == -1  # VG_ERR_INVALID_ARG
    assert b"NULL index" in lib.vg_last_error()


def test_header_declares_insert():
    h = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR (\d+)", h).group(1) == "13"
    decl = re.search(r"int32_t vg_hnsw_insert\(([^)]*)\);", h)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert args == ["vg_index *idx", "const float *rows", "int64_t count", "int32_t m", "int32_t ef_construction",
                    "int32_t max_batch", "int32_t growth_div", "void *stream"]
    # the parity contract the GPU tests rely on is stated next to the declaration
    assert "a batch boundary of the one-call schedule" in h


def test_cpp_and_go_mirrors_name_insert():
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert re.search(r"void InsertHNSW\(const float \*rows, int64_t count, int m = 32, int ef = 300, int maxBatch = 8192, "
                     r"int growthDiv = 32\)", hpp)
    assert "vg_hnsw_insert(h_, rows, count, m, ef, maxBatch, growthDiv, nullptr)" in hpp
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    assert "func (r *Resident) InsertHNSW(rows []float32, m, efConstruction int) error" in go
    assert "C.vg_hnsw_insert(" in go


def test_python_checks_shape_and_dtype():
    import numpy as np
    import pytest
    from vecgo_amd import api

    idx = api.Index.__new__(api.Index)  # no device needed: the checks run before the library is called
    idx.dim, idx.n = 8, 0
    with pytest.raises(ValueError):
        idx.insert_hnsw(np.zeros((3, 7), np.float32))
    with pytest.raises(ValueError):
        idx.insert_hnsw(np.zeros(8, np.float32))
    with pytest.raises(TypeError):
        idx.insert_hnsw(np.zeros((3, 8), np.float64))
