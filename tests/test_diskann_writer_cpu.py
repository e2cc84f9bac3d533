"""vg_diskann_build / vg_segment_write_diskann without a GPU: the numpy restatement of diskann.Writer.Flush the GPU tests compare
against (tests/diskann_writer_ref.py) checked field by field against diskann/format.go's offsets and section by section against
tests/segfile.py's (padded, metadata-free) writer, and the new entry points' declarations, exports, bindings and NULL-handle
refusals.

vg_segment_diskann_image_size takes a vg_index, which needs a device: its equality with the helper's image length is asserted
in tests/test_gpu_diskann_build.py."""
import ctypes as C
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from tests import diskann_writer_ref as ref
from tests import segfile

ROOT = Path(__file__).resolve().parents[1]
NEW = ("vg_diskann_build", "vg_segment_diskann_image_size", "vg_segment_write_diskann")
KINDS = ("none", "pq", "rabitq", "int4")


def small_case(kind):
    """n = 7, dim = 5, r = 3; PQ with m = 5 (35 code bytes: odd), INT4 with 3 bytes per row, RaBitQ with 12"""
    rng = np.random.default_rng(len(kind))
    n, dim, r = 7, 5, 3
    x = rng.standard_normal((n, dim)).astype(np.float32)
    g = rng.integers(0, n, (n, r)).astype(np.uint32)
    g[2, 1] = g[5, 0] = ref.EMPTY                  # empty slots in the middle of a row
    kw, seg_kw = {}, {}
    if kind == "pq":
        m = 5
        sc, of = rng.random(m).astype(np.float32), rng.standard_normal(m).astype(np.float32)
        cb = rng.integers(-128, 128, m * 256 * (dim // m), dtype=np.int8)
        codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
        kw = dict(quant=ref.QUANT_PQ, pq_m=m, codes=codes, pq_scales=sc, pq_offsets=of, pq_codebooks=cb)
        seg_kw = dict(pq=(m, 256, sc, of, cb), pq_codes=codes)
    elif kind == "rabitq":
        codes = rng.integers(0, 256, (n, 12), dtype=np.uint8)
        kw = dict(quant=ref.QUANT_RABITQ, codes=codes)
        seg_kw = dict(rabitq_codes=codes)
    elif kind == "int4":
        mn, df = x.min(0), x.max(0) - x.min(0)
        codes = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        kw = dict(quant=ref.QUANT_INT4, codes=codes, int4_min=mn, int4_diff=df)
        seg_kw = dict(int4=(mn, df, codes))
    return n, dim, r, x, g, kw, seg_kw


@pytest.mark.parametrize("kind", KINDS)
def test_helper_image(kind):
    n, dim, r, x, g, kw, seg_kw = small_case(kind)
    ids = np.arange(n, dtype=np.uint64) + (1 << 40)
    md = np.arange(n + 1, dtype="<u8").tobytes() + b"abcdefg"          # 71 bytes
    mi = b"\x01\x03key"
    img = ref.image(0x1122334455, x, dim, 2, g, 4, search_list=77, compression=1, ids=ids, metadata=md, metadata_index=mi, **kw)
    sec = ref.sections(x, dim, g, ids=ids, metadata=md, metadata_index=mi, **{k: v for k, v in kw.items() if k != "pq_m"})
    quant = kw.get("quant", ref.QUANT_NONE)
    # every header field at the offset format.go:51-78 encodes it
    assert struct.unpack_from("<I", img, 0)[0] == 0x4449534B and struct.unpack_from("<I", img, 4)[0] == 2
    assert struct.unpack_from("<Q", img, 8)[0] == 0x1122334455
    assert struct.unpack_from("<I", img, 16)[0] == n and struct.unpack_from("<I", img, 20)[0] == dim and img[24] == 2
    assert struct.unpack_from("<I", img, 25)[0] == r and struct.unpack_from("<I", img, 29)[0] == 77 and struct.unpack_from("<I", img, 33)[0] == 4
    assert img[37] == quant == {"none": 0, "pq": 1, "rabitq": 5, "int4": 6}[kind]
    assert struct.unpack_from("<HH", img, 38) == ((5, 256) if kind == "pq" else (0, 0))
    assert img[42] == 1 and img[43:48] == bytes(5) and img[124:160] == bytes(36)
    offs = dict(zip(ref._OFFSETS, (struct.unpack_from("<Q", img, 48 + 8 * i)[0] for i in range(9))))
    assert offs == {k: v for k, v in ref.parse_header(img).items() if k in offs}
    # running sums, no gaps; an absent section's offset is 0
    at = ref.HEADER_SIZE
    assert offs["vector_off"] == at
    at += n * dim * 4
    assert offs["graph_off"] == at
    at += n * r * 4
    code_bytes = {"none": 0, "pq": 35, "rabitq": 84, "int4": 21}[kind]
    assert offs["pq_codes_off"] == (at if kind in ("pq", "int4") else 0)
    assert offs["bq_codes_off"] == (at if kind == "rabitq" else 0)
    at += code_bytes
    param_bytes = {"none": 0, "pq": 5 * 8 + 5 * 256, "rabitq": 0, "int4": 4 + dim * 8}[kind]
    assert offs["pq_codebook_off"] == (at if param_bytes else 0)
    at += param_bytes
    assert offs["pk_off"] == at
    at += n * 8
    assert offs["metadata_off"] == at
    at += len(md)
    assert offs["block_stats_off"] == 0 and offs["metadata_index_off"] == at
    assert len(img) == at + len(mi)
    assert code_bytes % 2 == 1 or kind in ("none", "rabitq")          # the odd-sized code sections the issue asks for
    # the checksum, and the body as the sections in order
    body = img[ref.HEADER_SIZE:]
    assert struct.unpack_from("<I", img, 120)[0] == segfile.crc32c_py(body) == ref.crc32c(body)
    assert body == b"".join(sec.values())
    # section by section against segfile's writer (which pads every section and has no metadata sections)
    other = segfile.write_diskann(x, g, 4, metric=2, segment_id=0x1122334455, search_list=77, **seg_kw)
    o = dict(zip(ref._OFFSETS, struct.unpack_from("<9Q", other, 48)))
    assert other[37] == img[37] and other[38:42] == img[38:42]
    for name, mine, theirs in (("vectors", offs["vector_off"], o["vector_off"]), ("graph", offs["graph_off"], o["graph_off"]),
                               ("codes", offs["pq_codes_off"] or offs["bq_codes_off"], o["pq_codes_off"] or o["bq_codes_off"]),
                               ("params", offs["pq_codebook_off"], o["pq_codebook_off"])):
        size = len(sec[name])
        assert (mine == 0) == (size == 0) == (theirs == 0) or name in ("vectors", "graph"), name
        assert img[mine:mine + size] == other[theirs:theirs + size] == sec[name], name
    assert other[o["pk_off"]:o["pk_off"] + n * 8] == np.arange(n, dtype="<u8").tobytes()     # (segfile writes 0 .. n-1)
    assert img[offs["pk_off"]:offs["pk_off"] + n * 8] == ids.astype("<u8").tobytes()
    assert img[offs["metadata_off"]:offs["metadata_index_off"]] == md and img[offs["metadata_index_off"]:] == mi


def test_nil_document_sections():
    n, dim, r, x, g, _, _ = small_case("none")
    img = ref.image(1, x, dim, 0, g, 0)
    h = ref.parse_header(img)
    assert h["search_list_size"] == 100 and h["compression"] == 1
    assert img[h["metadata_off"]:h["metadata_index_off"]] == bytes(8 * (n + 1))
    assert img[h["metadata_index_off"]:] == b"\x00" and len(img) == h["metadata_index_off"] + 1
    assert img[h["pk_off"]:h["metadata_off"]] == np.arange(n, dtype="<u8").tobytes()
    assert ref.int4_params(3, [1, 2, 3], [4, 5, 6]) == struct.pack("<I6f", 3, 1, 2, 3, 4, 5, 6)
    assert ref.crc32c(b"123456789") == 0xE3069283


# ---- the library's new surface (fails before the feature) --------------------------------------------------------------
def test_python_binding_has_the_methods():
    import vecgo_amd
    assert callable(getattr(vecgo_amd.Index, "diskann_build", None))
    assert callable(getattr(vecgo_amd.Index, "write_diskann_segment", None))


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
    assert lib.vg_abi_minor() == 13


def test_go_and_cpp_mirrors_bind_them():
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, f"{name} has no Go binding"
        assert f"{name}(" in hpp, f"{name} has no C++ mirror"
    assert "func (r *Resident) DiskANNBuild(" in go and "func (r *Resident) WriteDiskANN(" in go
    assert "DiskANNBuild(" in hpp and "WriteDiskANN(" in hpp


def test_null_handles_are_refused():
    from vecgo_amd import _lib
    lib = _lib.load()
    lib.vg_segment_diskann_image_size.restype = C.c_int64
    perm = np.zeros(4, np.uint32)
    used = C.c_int32(9)
    assert lib.vg_diskann_build(None, C.c_int32(8), C.c_int32(16), C.c_float(1.2), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_uint64(1),
                                C.c_int32(1), C.c_int32(1), None, None, C.c_void_p(perm.ctypes.data), None, C.byref(used), None) == -1
    assert b"NULL index" in lib.vg_last_error() and not perm.any() and used.value == 9
    assert lib.vg_segment_diskann_image_size(None, C.c_int64(-1), C.c_int64(-1)) == -1
    buf = np.zeros(256, np.uint8)
    written = C.c_int64(5)
    assert lib.vg_segment_write_diskann(None, C.c_uint64(1), C.c_int32(0), C.c_int32(1), None, None, C.c_int64(0), None, C.c_int64(0),
                                        C.c_void_p(buf.ctypes.data), C.c_int64(buf.size), C.byref(written), None) == -1
    assert written.value == 0 and not buf.any()
