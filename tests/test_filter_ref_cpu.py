"""Filters on the device, the part that needs no GPU: tests/filter_ref.py against cases from the reference's own tests
(tests/golden/filter_kats.json, each citing its source line), the Python packing of clauses / offsets / sets against a
hand-written layout, and the header's new declarations."""
import json
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from tests import filter_ref as ref

ROOT = Path(__file__).resolve().parents[1]
KATS = json.loads((ROOT / "tests" / "golden" / "filter_kats.json").read_text())["cases"]
NEW = ("vg_columns_create", "vg_columns_destroy", "vg_columns_set_f64", "vg_columns_set_codes", "vg_columns_drop",
       "vg_filter_evaluate", "vg_mask_combine", "vg_mask_popcount")


def kat_columns(case):
    cols = ref.RefColumns(case["rows"])
    for field, c in case["columns"].items():
        if c["kind"] == "f64":
            cols.set_f64(int(field), c["values"], c.get("present"))
        else:
            cols.set_codes(int(field), c["codes"])
    return cols


@pytest.mark.parametrize("case", KATS, ids=lambda c: c["name"])
def test_helper_matches_the_reference_cases(case):
    assert re.match(r"internal/metadata/\w+_test\.go:\d+", case["source"])
    filters = [tuple(f) for f in case["filters"]]
    got = np.flatnonzero(ref.match_set(kat_columns(case), filters))
    assert got.tolist() == case["want_rows"] and got.size == case["want_count"]
    masks, counts = ref.evaluate(kat_columns(case), [filters])
    assert counts.tolist() == [case["want_count"]]
    assert np.flatnonzero(np.unpackbits(masks[0], bitorder="little")).tolist() == case["want_rows"]   # tail bits zero


def test_there_are_a_dozen_cases_from_both_files():
    assert len(KATS) >= 12
    assert {c["source"].split(":")[0].rsplit("/", 1)[1] for c in KATS} == {"numeric_index_test.go", "unified_test.go"}


def test_helper_semantics_the_cases_do_not_reach():
    cols = ref.RefColumns(6)
    cols.set_f64(0, [1.0, np.nan, -0.0, 0.0, np.inf, 5.0], [True, True, True, True, True, False])
    cols.set_codes(1, [3, ref.INVALID_ID, 3, 4, 5, 3])
    rows = lambda *f, **k: np.flatnonzero(ref.match_set(cols, list(f), **k)).tolist()
    assert rows() == [0, 1, 2, 3, 4, 5]                                 # an empty set matches every row
    assert rows((7, "eq", 1.0)) == [] and rows((7, "ne", 1.0)) == []    # no such column: nothing
    assert rows((0, "ne", 1.0)) == [1, 2, 3, 4]                         # a stored NaN is kept by ne; the absent row is not
    assert rows((0, "eq", np.nan)) == [] and rows((0, "lte", np.nan)) == []
    assert rows((0, "ne", np.nan)) == [0, 1, 2, 3, 4]                   # a NaN filter value: every present row under ne
    assert rows((0, "eq", 0.0)) == [2, 3] and rows((0, "lt", 0.0)) == []   # -0 == +0
    assert rows((0, "gt", 1.0)) == [4] and rows((0, "gte", 1.0)) == [0, 4]
    assert rows((1, "eq", 3)) == [0, 2, 5] and rows((1, "eq", ref.INVALID_ID)) == []
    assert rows((1, "in", [])) == [] and rows((1, "in", [4, 4, 9, 3])) == [0, 2, 3, 5]
    assert rows((1, "in", [ref.INVALID_ID])) == []
    assert rows((1, "eq", 3), (0, "gte", 0.0)) == [0, 2]
    assert rows((1, "eq", 3), deleted=[True, False, False, False, False, False]) == [2, 5]
    with pytest.raises(ValueError):
        rows((1, "lt", 3))
    m, c = ref.evaluate(cols, [[], [(1, "eq", 4)]])
    assert m.tolist() == [[0b00111111], [0b00001000]] and c.tolist() == [6, 1]


def test_python_packing_matches_a_hand_written_layout():
    import vecgo_amd as vg
    assert vg.FILTER_CLAUSE.itemsize == 32
    clauses, off, sets = vg.pack_filter_sets([
        [(3, "lt", 2.5), (63, vg.FilterOp.IN, [7, 7, 9])],
        [],
        [(0, 0, 5), (1, "in", []), (2, "in", [1])],
    ])
    assert off.dtype == np.int32 and off.tolist() == [0, 2, 2, 5]
    assert sets.dtype == np.uint32 and sets.tolist() == [7, 7, 9, 1]
    inv = 0xFFFFFFFF
    #                        field op  value code set_begin set_count reserved
    want = b"".join(struct.pack("<iidIiii", *r) for r in [
        (3, 2, 2.5, inv, 0, 0, 0),
        (63, 6, 0.0, inv, 0, 3, 0),
        (0, 0, 5.0, 5, 0, 0, 0),
        (1, 6, 0.0, inv, 3, 0, 0),
        (2, 6, 0.0, inv, 3, 1, 0),
    ])
    assert len(want) == 5 * 32 and clauses.tobytes() == want
    empty = vg.pack_filter_sets([])
    assert empty[0].size == 0 and empty[1].tolist() == [0] and empty[2].size == 0
    assert [int(o) for o in vg.FilterOp] == list(range(7)) and [o.name.lower() for o in vg.FilterOp] == list(ref.OPS)


def test_header_declares_the_new_surface():
    from vecgo_amd import _lib
    import vecgo_amd as vg
    text = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR 13\b", text)
    note = text[text.index("Added at minor 13 without a bump"):text.index("#define VG_ABI_MINOR")]
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.declared_symbols(), name
        assert hasattr(lib, name), f"libvecgo_hip.so does not export {name}"
    assert "vg_filter_evaluate" in note and "vg_mask_popcount" in note and "Likewise" in note
    body = re.search(r"typedef struct vg_filter_clause \{(.*?)\} vg_filter_clause;", text, flags=re.S).group(1)
    assert [w for w in re.findall(r"\b(field|op|value|code|set_begin|set_count|reserved)\b", re.sub(r"/\*.*?\*/", "", body))] == \
        ["field", "op", "value", "code", "set_begin", "set_count", "reserved"]
    assert re.search(r"enum \{ VG_FILTER_EQ = 0, VG_FILTER_NE, VG_FILTER_LT, VG_FILTER_LTE, VG_FILTER_GT, VG_FILTER_GTE, VG_FILTER_IN \}", text)
    assert re.search(r"enum \{ VG_MASK_AND = 0, VG_MASK_ANDNOT, VG_MASK_OR, VG_MASK_XOR \}", text)
    assert int(re.search(r"#define VG_FILTER_TILE_ROWS (\d+)", text).group(1)) == vg.FILTER_TILE_ROWS
    for cite in ("unified.go:279-416", "numeric_index.go:1020-1037", "compareFloat64", "bitmap.go:26-48"):
        assert cite in text, cite
    enqueue = text[text.index("Enqueue-only entry points"):text.index("These WAIT for")]
    assert "vg_filter_evaluate" in enqueue


def test_bindings_name_the_new_surface():
    import vecgo_amd as vg
    go = (ROOT / "go" / "segment" / "filter_hip.go").read_text()
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    api = (ROOT / "vecgo_amd" / "api.py").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, name
        assert f"{name}(" in hpp, name
        assert f"_lib.{name}(" in api, name
    for fn in ("SetFloat64", "SetCodes", "Drop", "EvaluateFilters"):
        assert re.search(rf"^func \([^)]*\) {fn}\(", go, flags=re.M), fn
    for name in ("Columns", "evaluate_filters", "mask_combine", "mask_popcount", "pack_filter_sets"):
        assert callable(getattr(vg, name)) and name in vg.__all__


def test_malformed_calls_are_refused_without_a_device():
    """every refusal here comes before the library touches a device"""
    import ctypes as C
    from vecgo_amd import _lib
    lib = _lib.load()
    out = C.c_void_p(0x1234)
    assert lib.vg_columns_create(None, C.c_int64(4), C.byref(out)) == -1 and out.value is None
    fake_ctx = C.c_void_p(0x10)   # never dereferenced below
    assert lib.vg_columns_create(fake_ctx, C.c_int64(-1), C.byref(out)) == -1
    assert lib.vg_columns_create(fake_ctx, C.c_int64(1 << 31), C.byref(out)) == -5 and b"2147483648" in lib.vg_last_error()
    assert lib.vg_columns_destroy(None) == 0
    assert lib.vg_columns_set_f64(None, C.c_int32(0), None, None, None) == -1
    assert lib.vg_columns_set_codes(None, C.c_int32(0), None, None) == -1
    assert lib.vg_columns_drop(None, C.c_int32(0)) == -1
    assert lib.vg_filter_evaluate(None, None, None, C.c_int64(1), None, C.c_int64(0), None, None, C.c_int64(0), None, None) == -1
    assert lib.vg_mask_combine(None, C.c_int32(0), None, C.c_int64(0), None, C.c_int64(0), C.c_int64(1), C.c_int64(8), None) == -1
    assert lib.vg_mask_combine(fake_ctx, C.c_int32(4), None, C.c_int64(0), None, C.c_int64(0), C.c_int64(1), C.c_int64(8), None) == -1
    assert b"unknown op 4" in lib.vg_last_error()
    assert lib.vg_mask_popcount(None, None, C.c_int64(0), C.c_int64(1), C.c_int64(8), None, None) == -1
