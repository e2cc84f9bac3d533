"""vg_index_merge / vecgo_amd.compact without a GPU: the numpy restatement of the compaction's Iterate loop the GPU tests
compare against (tests/compact_ref.py) checked against a literal double loop, the choice of writer against the reference's
arithmetic, and the new entry point's declaration, export, bindings and NULL-argument refusals."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import compact_ref as ref

ROOT = Path(__file__).resolve().parents[1]
NEW = "vg_index_merge"


def literal_loop(sources, bitmaps):
    """compaction.go:173-218 word for word: segments in order, rows in order, `ts != nil && ts.Contains(rowID)` skips"""
    rows, moves, count = [], {}, 0
    new_source, new_row = [], []
    for s, seg in enumerate(sources):
        ts = bitmaps[s] if bitmaps is not None else None
        for row_id in range(len(seg)):
            if ts is not None and (ts[row_id >> 3] >> (row_id & 7)) & 1:
                continue
            rows.append(seg[row_id])
            moves[(s, row_id)] = count
            new_source.append(s)
            new_row.append(row_id)
            count += 1
    old_to_new = [moves.get((s, r), ref.INVALID) for s, seg in enumerate(sources) for r in range(len(seg))]
    dim = sources[0].shape[1]
    return (np.array(rows, np.float32).reshape(-1, dim), np.array(old_to_new, np.uint32), np.array(new_source, np.int32),
            np.array(new_row, np.uint32))


def _cases():
    rng = np.random.default_rng(3)

    def make(sizes, dim, p):
        src = [rng.standard_normal((n, dim)).astype(np.float32) for n in sizes]
        bm = [np.packbits(rng.random(n) < p, bitorder="little") for n in sizes]
        return src, bm
    yield "one source, nothing deleted", make([40], 3, 0.0)[0], None
    yield "a None bitmap among others", *(lambda s, b: (s, [b[0], None, b[2]]))(*make([9, 17, 8], 2, 0.5))
    yield "empty and one-row sources", *make([25, 0, 33, 1], 4, 0.3)
    yield "everything deleted", *make([7, 12], 2, 1.1)
    yield "many small", *make(list(rng.integers(0, 30, 12)), 1, 0.4)


@pytest.mark.parametrize("name,sources,bitmaps", list(_cases()), ids=[c[0] for c in _cases()])
def test_helper_is_the_loop(name, sources, bitmaps):
    got = ref.merge(sources, bitmaps)
    want = literal_loop(sources, bitmaps)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()


def test_helper_ignores_bits_past_the_last_row_and_takes_bool():
    x = [np.arange(20, dtype=np.float32).reshape(10, 2)]
    bm = np.array([0b00000101, 0b11111110], np.uint8)   # rows 0, 2, 9 deleted; bits 10..15 are not rows
    rows, o2n, ns, nr = ref.merge(x, [bm])
    assert list(nr) == [1, 3, 4, 5, 6, 7, 8] and list(o2n) == [ref.INVALID, 0, ref.INVALID, 1, 2, 3, 4, 5, 6, ref.INVALID]
    same = ref.merge(x, [ref.unpack(bm, 10)])
    assert all(np.array_equal(a, b) for a, b in zip(same, (rows, o2n, ns, nr)))


def test_compose_follows_a_permutation():
    rng = np.random.default_rng(5)
    x = [rng.standard_normal((n, 2)).astype(np.float32) for n in (13, 6)]
    rows, o2n, ns, nr = ref.merge(x, [rng.random(13) < 0.4, None])
    perm = rng.permutation(len(rows)).astype(np.uint32)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size, dtype=np.uint32)
    final, fs, fr = ref.compose(o2n, ns, nr, perm, inv)
    built = rows[perm]
    off = [0, 13]
    for g, j in enumerate(final):
        s, r = (0, g) if g < 13 else (1, g - 13)
        if j == ref.INVALID:
            assert o2n[g] == ref.INVALID
        else:
            assert np.array_equal(built[j], x[s][r]) and fs[j] == s and fr[j] == r and final[off[s] + r] == j


# ---- the policy --------------------------------------------------------------------------------------------------------
def reference_arithmetic(total_rows, configured):
    """compaction.go:104-140 in Go's types: uint32 counts, integer division"""
    threshold = np.uint32(10000)
    if configured > 0:
        threshold = np.uint32(configured)
    if np.uint32(total_rows) >= threshold:
        return "diskann", 0
    k = int(np.uint32(total_rows) // np.uint32(8192))
    return "flat", max(k, 1)


def test_compaction_plan_is_the_engines():
    import vecgo_amd as vg
    for plan in (vg.compaction_plan, ref.plan):
        # the partition count's seams: k stays 1 up to 16383 rows, 16384 gives 2.  At the default threshold a total from
        # 10000 up never reaches the flat writer (16383 >= 10000 is DiskANN, :113), so the totals above it are planned
        # with the threshold out of the way
        for total in (0, 8191, 8192, 9999):
            assert plan(total) == ("flat", 1), total
        assert plan(16383, 100000) == ("flat", 1)
        assert plan(16384, 100000) == ("flat", 2)
        assert plan(10000) == ("diskann", 0)
        assert plan(16383) == ("diskann", 0)
        assert plan(9999, 0) == plan(9999, -5) == ("flat", 1)        # a threshold of 0 or less is the default
        assert plan(99999, 100000) == ("flat", 12) and plan(100000, 100000) == ("diskann", 0)
        assert plan(5, 5) == ("diskann", 0) and plan(4, 5) == ("flat", 1)
        for total in (0, 1, 8191, 8192, 9999, 10000, 16383, 16384, 24576, 99999, 100000, 1 << 20):
            for configured in (0, 1, 2000, 10000, 100000, 1 << 30):
                assert plan(total, configured) == reference_arithmetic(total, configured), (total, configured)


# ---- the library's new surface -----------------------------------------------------------------------------------------
def test_declared_exported_and_named_in_the_minor_note():
    from vecgo_amd import _lib
    text = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR 13\b", text)
    note = text[text.index("Added at minor 13 without a bump"):text.index("#define VG_ABI_MINOR")]
    lib = _lib.load()
    assert NEW in _lib.declared_symbols(), f"{NEW} is not declared in include/vecgo_hip.h"
    assert hasattr(lib, NEW), f"libvecgo_hip.so does not export {NEW}"
    assert NEW in note and "symbol lookup" in note
    assert "compaction.go:173-218" in text
    assert lib.vg_abi_minor() == 13


def test_bindings_name_it():
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    api = (ROOT / "vecgo_amd" / "api.py").read_text()
    assert f"C.{NEW}(" in go and "func Merge(sources []*Resident, deleted [][]byte)" in go and "func Compact(" in go
    assert f"{NEW}(" in hpp
    assert f"_lib.{NEW}(" in api
    import vecgo_amd as vg
    for name in ("merge_indexes", "compaction_plan", "compact"):
        assert callable(getattr(vg, name)) and name in vg.__all__


def test_null_arguments_are_refused():
    from vecgo_amd import _lib
    lib = _lib.load()
    fn = lib.vg_index_merge
    out = C.c_void_p(0x1234)
    maps = np.full(4, 7, np.uint32)
    one = (C.c_void_p * 1)(None)
    pm = C.c_void_p(maps.ctypes.data)
    fake_ctx = C.c_void_p(0x10)   # never dereferenced: every refusal below comes before the context is used

    assert fn(None, one, None, C.c_int32(1), C.byref(out), pm, None, None, None) == -1          # NULL context
    assert out.value is None and b"NULL" in lib.vg_last_error()
    out = C.c_void_p(0x1234)
    assert fn(fake_ctx, None, None, C.c_int32(1), C.byref(out), pm, None, None, None) == -1     # NULL sources
    assert out.value is None
    assert fn(fake_ctx, one, None, C.c_int32(1), None, pm, None, None, None) == -1              # NULL out
    out = C.c_void_p(0x1234)
    assert fn(fake_ctx, one, None, C.c_int32(0), C.byref(out), pm, None, None, None) == -1      # no sources
    assert out.value is None and b"n_sources" in lib.vg_last_error()
    out = C.c_void_p(0x1234)
    assert fn(fake_ctx, one, None, C.c_int32(-3), C.byref(out), pm, None, None, None) == -1
    assert out.value is None
    out = C.c_void_p(0x1234)
    assert fn(fake_ctx, one, None, C.c_int32(1), C.byref(out), pm, None, None, None) == -1      # a NULL source
    assert out.value is None and b"source 0 is NULL" in lib.vg_last_error()
    assert np.all(maps == 7)                                                                    # nothing written
