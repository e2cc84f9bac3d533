"""vg_hnsw_compact without a GPU: the symbol is exported and declared with its argument list, the minor version is unchanged,
a NULL index is refused, the C++ and Go mirrors name the call, the Python wrapper checks its arguments first — and the
plain-Python restatement the GPU tests compare with (tests/hnsw_compact_ref.py) holds compact_test.go's invariants."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_abi_exports_and_null_index():
    from vecgo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vg_hnsw_compact")
    assert lib.vg_abi_minor() == 13
    stats = (C.c_int64 * 4)()
    st = lib.vg_hnsw_compact(None, 300, 8192, stats, None)
    assert st == -1  # VG_ERR_INVALID_ARG
    assert b"NULL index" in lib.vg_last_error()


def test_header_declares_compact():
    h = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR (\d+)", h).group(1) == "13"
    decl = re.search(r"int32_t vg_hnsw_compact\(([^)]*)\);", h)
    assert decl is not None
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["vg_index *idx", "int32_t ef_construction", "int32_t max_batch", "vg_hnsw_compact_stats *stats", "void *stream"]
    body = re.search(r"typedef struct vg_hnsw_compact_stats \{(.*?)\} vg_hnsw_compact_stats;", h, flags=re.S).group(1)
    assert re.findall(r"int64_t (\w+);", body) == ["repaired_nodes", "repaired_lists", "pruned_links", "cleared_nodes"]
    minor = h[h.index("Added at minor 13 without a bump"):h.index("#define VG_ABI_MINOR")]
    assert "vg_hnsw_compact" in minor  # found by symbol lookup until the next bump
    assert "ascending id order" in h   # the rule the reference leaves open is stated next to the declaration


def test_cpp_and_go_mirrors_name_compact():
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert re.search(r"CompactHNSW\(int ef = 300, int maxBatch = 8192\)", hpp)
    assert "vg_hnsw_compact(h_, ef, maxBatch, &stats, nullptr)" in hpp
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    assert "func (r *Resident) CompactHNSW(efConstruction int) error" in go
    assert "C.vg_hnsw_compact(" in go


def test_python_checks_arguments_first():
    from vecgo_amd import api

    idx = api.Index.__new__(api.Index)  # no device, no library handle: the checks run before the library is called
    with pytest.raises(ValueError):
        idx.compact_hnsw(max_batch=0)
    with pytest.raises(ValueError):
        idx.compact_hnsw(ef_construction=-1)
    with pytest.raises(ValueError):
        idx.compact_hnsw(ef_construction=1025)
    with pytest.raises(TypeError):
        idx.compact_hnsw(ef_construction=300.0)
    with pytest.raises(TypeError):
        idx.compact_hnsw(max_batch="8192")


# ---- the restatement on compact_test.go's shape: 1000 x 16 uniform rows, M 16, EF 200, even ids deleted ----
@pytest.fixture(scope="module")
def compacted():
    from oracle import oracle as o
    from tests import hnsw_compact_ref as ref

    rng = np.random.default_rng(42)
    n, dim, m = 1000, 16, 16
    base = rng.random((n, dim), dtype=np.float32)
    l0, upper, entry = o.hnsw_build(base, dim, m=m, ef=200)
    dead = (np.arange(n) % 2) == 0
    runs = {mb: ref.compact(base, dim, l0, upper, entry, dead, m, ef=200, max_batch=mb) for mb in (1, 64)}
    return dict(base=base, l0=l0, upper=upper, entry=entry, dead=dead, runs=runs)


def test_restatement_distances_are_the_pair_kernel():
    from oracle import oracle as o
    rng = np.random.default_rng(3)
    base = rng.standard_normal((37, 24)).astype(np.float32)
    every = np.arange(37, dtype=np.uint32)
    row = o.rerank_f32(base, 24, base[5], every, o.METRIC_L2)
    drow = o.rerank_f32(base, 24, base[5], every, o.METRIC_DOT)
    for j in range(37):  # the rows the restatement caches are the single-pair kernels, bit for bit and symmetric
        assert row[j].view(np.uint32) == o.l2(base[5], base[j]).view(np.uint32)
        assert row[j].view(np.uint32) == o.l2(base[j], base[5]).view(np.uint32)
        assert drow[j].view(np.uint32) == o.dot(base[5], base[j]).view(np.uint32)
        assert drow[j].view(np.uint32) == o.dot(base[j], base[5]).view(np.uint32)


@pytest.mark.parametrize("max_batch", [1, 64])
def test_restatement_invariants(compacted, max_batch):
    from tests import hnsw_compact_ref as ref
    l0, upper, entry, stats, detail = compacted["runs"][max_batch]
    dead = compacted["dead"]
    assert ref.invariants(l0, upper, dead) == []
    assert entry == compacted["entry"]
    assert stats["repaired_nodes"] > 0 and stats["repaired_lists"] > 0
    assert stats["cleared_nodes"] == int(dead.sum())  # every node of a built graph holds a link
    before = compacted["l0"]
    dead_links = sum(int(dead[x]) for v in range(before.shape[0]) if not dead[v] for x in before[v] if x != ref.INVALID)
    assert stats["pruned_links"] >= dead_links  # layer 0 alone; kept tombstones are pruned exactly once
    # the inputs are untouched
    assert l0 is not compacted["l0"] and not np.array_equal(l0, compacted["l0"])


def test_restatement_batches_agree_on_the_repaired_nodes(compacted):
    a, b = compacted["runs"][1][4], compacted["runs"][64][4]
    assert a["need"] == b["need"] and len(a["need"]) > 0


def test_restatement_no_tombstones_is_a_no_op(compacted):
    from tests import hnsw_compact_ref as ref
    c = compacted
    l0, upper, entry, stats, _ = ref.compact(c["base"], 16, c["l0"], c["upper"], c["entry"], np.zeros(1000, np.bool_), 16, ef=200)
    assert np.array_equal(l0, c["l0"]) and all(np.array_equal(x[1], y[1]) for x, y in zip(upper, c["upper"]))
    assert stats == dict(repaired_nodes=0, repaired_lists=0, pruned_links=0, cleared_nodes=0)
