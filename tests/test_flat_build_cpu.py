"""vg_flat_build / vg_segment_write_flat / vg_crc32c_device without a GPU: the numpy restatement of flat.Writer.Flush the GPU
tests compare against (tests/flat_writer_ref.py) checked against itself, and the new entry points' declarations, exports, Go
bindings and NULL-handle refusals.

vg_segment_flat_image_size takes a vg_index, and an index needs a context, which needs a device: its equality with the
helper's image length (none / SQ8 / PQ x partitioned / not, rows = 0) is asserted in tests/test_gpu_flat_build.py, here the
helper's own length arithmetic is."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import flat_writer_ref as ref
from tests import segfile

ROOT = Path(__file__).resolve().parents[1]
NEW = ("vg_flat_build", "vg_segment_flat_image_size", "vg_segment_write_flat", "vg_crc32c_device")


# ---- the helper against itself -----------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(11)
    yield "random", rng.integers(0, 7, 5000), 7
    yield "one partition of many", np.full(1000, 3), 9
    yield "empty partitions", rng.choice([0, 4, 5, 11], 3000), 12
    yield "descending ids", np.arange(999, -1, -1) // 10, 100
    yield "skewed", np.minimum(rng.geometric(0.3, 4000) - 1, 121), 122
    yield "more partitions than LDS counters", rng.integers(0, 5000, 20000), 5000
    yield "no rows", np.zeros(0, np.int64), 4


@pytest.mark.parametrize("name,assign,k", list(_cases()), ids=[c[0] for c in _cases()])
def test_fill_is_a_stable_sort(name, assign, k):
    perm, inv, off = ref.group(assign, k)
    want = np.argsort(np.asarray(assign), kind="stable")
    assert np.array_equal(perm, want)
    assert np.array_equal(inv[perm], np.arange(assign.size))
    assert np.array_equal(off, np.searchsorted(np.asarray(assign)[want], np.arange(k + 1)))
    assert off[k] == assign.size and np.all(np.diff(off.astype(np.int64)) >= 0)


def test_nil_document_sections():
    assert ref.nil_metadata(0) == b"" and ref.nil_block_stats(0) == b"\x00"
    assert ref.nil_metadata(3) == bytes(16)
    assert ref.nil_block_stats(1) == b"\x01\x01\x00" and ref.nil_block_stats(1024) == b"\x01\x01\x00"
    assert ref.nil_block_stats(1025) == b"\x02\x01\x00\x01\x00"
    big = ref.nil_block_stats(200 * 1024)          # 200 blocks: a two-byte uvarint
    assert big[:2] == b"\xc8\x01" and len(big) == 2 + 400
    assert ref.crc32c(b"123456789") == 0xE3069283 == segfile.crc32c_py(b"123456789")


# (Flush never partitions or quantizes an empty segment, writer.go:105, :178: rows = 0 comes plain)
@pytest.mark.parametrize("rows,k,quant", [(0, 0, ref.QUANT_NONE)] + [(37, k, q) for k in (0, 5)
                                                                     for q in (ref.QUANT_NONE, ref.QUANT_SQ8, ref.QUANT_PQ)])
def test_header_offsets_parse_back(rows, k, quant):
    rng = np.random.default_rng(rows + k + quant)
    dim, m = 24, 3
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    kw = {}
    if k:
        kw.update(centroids=rng.standard_normal((k, dim)).astype(np.float32),
                  part_offsets=np.linspace(0, rows, k + 1).astype(np.uint32))
    if quant == ref.QUANT_SQ8:
        kw.update(sq_mins=x.min(0), sq_maxs=x.max(0), codes=rng.integers(0, 256, (rows, dim), dtype=np.uint8))
    if quant == ref.QUANT_PQ:
        kw.update(pq_m=m, pq_scales=np.ones(m, np.float32), pq_offsets=np.zeros(m, np.float32),
                  pq_codebooks=rng.integers(-128, 128, m * 256 * (dim // m), dtype=np.int8),
                  codes=rng.integers(0, 256, (rows, m), dtype=np.uint8))
    md = np.arange(rows + 1, dtype="<u4").tobytes() + b"x" * rows if rows else b""
    img = ref.image(77, x, dim, 2, quant=quant, metadata=md, **kw)
    h = ref.parse_header(img)
    assert (h["segment_id"], h["rows"], h["dim"], h["metric"], h["num_partitions"], h["quant"]) == (77, rows, dim, 2, k, quant)
    sizes = [k * dim * 4, (k + 1) * 4 if k else 0,
             {ref.QUANT_NONE: 0, ref.QUANT_SQ8: dim * 8, ref.QUANT_PQ: 8 + m * 8 + m * 256 * (dim // m)}[quant],
             {ref.QUANT_NONE: 0, ref.QUANT_SQ8: rows * dim, ref.QUANT_PQ: rows * m}[quant], rows * dim * 4, rows * 8, len(md)]
    at = ref.HEADER_SIZE
    for field, size in zip(ref._FIELDS, sizes):            # no padding: each section starts where the last one ended
        assert h[field] == at, field
        at += size
    assert h["block_stats_off"] == at and len(img) == at + len(ref.nil_block_stats(rows))
    assert h["checksum"] == segfile.crc32c_py(img[ref.HEADER_SIZE:])
    assert img[h["vector_off"]:h["vector_off"] + rows * dim * 4] == x.tobytes()
    assert img[h["pk_off"]:h["pk_off"] + rows * 8] == np.arange(rows, dtype="<u8").tobytes()


# ---- the library's new surface -----------------------------------------------------------------------------------------
def test_declared_exported_and_named_in_the_minor_note():
    from vecgo_amd import _lib
    text = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR 13\b", text)
    note = text[text.index("Added at minor 13 without a bump"):text.index("#define VG_ABI_MINOR")]
    lib = _lib.load()
    declared = set(_lib.declared_symbols())
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/vecgo_hip.h"
        assert hasattr(lib, name), f"libvecgo_hip.so does not export {name}"
        assert name in note, f"{name} is not in the minor-13 note"
    assert "symbol lookup" in note
    assert lib.vg_abi_minor() == 13


def test_go_and_cpp_mirrors_bind_them():
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, f"{name} has no Go binding"
        assert f"{name}(" in hpp, f"{name} has no C++ mirror"


def test_null_handles_are_refused():
    from vecgo_amd import _lib
    lib = _lib.load()
    lib.vg_segment_flat_image_size.restype = C.c_int64
    perm = np.zeros(4, np.uint32)
    assert lib.vg_flat_build(None, C.c_int32(4), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_uint64(1), None, None,
                             C.c_void_p(perm.ctypes.data), None, None) == -1
    assert b"NULL index" in lib.vg_last_error() and not perm.any()
    assert lib.vg_segment_flat_image_size(None, C.c_int64(-1), C.c_int64(-1)) == -1
    buf = np.zeros(256, np.uint8)
    written = C.c_int64(5)
    assert lib.vg_segment_write_flat(None, C.c_uint64(1), None, None, C.c_int64(0), None, C.c_int64(0), C.c_void_p(buf.ctypes.data),
                                     C.c_int64(buf.size), C.byref(written), None) == -1
    assert written.value == 0 and not buf.any()
    out = C.c_uint32(9)
    assert lib.vg_crc32c_device(None, C.c_void_p(buf.ctypes.data), C.c_int64(16), C.byref(out), None) == -1
    assert lib.vg_crc32c_device(None, None, C.c_int64(0), None, None) == -1
