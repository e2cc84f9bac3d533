"""diskann.Writer.Flush restated in numpy for the tests of vg_diskann_build / vg_segment_write_diskann: the file image
(internal/segment/diskann/writer.go:645-856, header fields diskann/format.go:19-47, encoded as :51-78).  Written from the
reference, section by section; unlike tests/segfile.py it pads nothing between sections and writes the two metadata sections,
because the reference writer does."""
from __future__ import annotations

import struct

import numpy as np

HEADER_SIZE = 160                       # format.go:49
MAGIC, VERSION = 0x4449534B, 2          # format.go:9-10
QUANT_NONE, QUANT_PQ, QUANT_RABITQ, QUANT_INT4 = 0, 1, 5, 6   # quantization.Type, types.go:6-14
EMPTY = 0xFFFFFFFF                      # writer.go:715 the sentinel of an unused slot

_OFFSETS = ("vector_off", "graph_off", "pq_codes_off", "bq_codes_off", "pq_codebook_off", "pk_off", "metadata_off",
            "block_stats_off", "metadata_index_off")


def nil_metadata(rows: int) -> bytes:
    """writer.go:797-823 with every w.metadata[i] nil: rows + 1 zero uint64 offsets, an empty blob"""
    return bytes(8 * (rows + 1))


def nil_metadata_index() -> bytes:
    """UnifiedIndex.WriteInvertedIndex of an empty index (internal/metadata/unified.go:1724-1733): uvarint(0 fields)"""
    return b"\x00"


def int4_params(dim: int, mins, diffs) -> bytes:
    """Int4Quantizer.MarshalBinary (quantization/int4.go:171-188)"""
    return struct.pack("<I", dim) + np.ascontiguousarray(mins, "<f4").tobytes() + np.ascontiguousarray(diffs, "<f4").tobytes()


def crc32c(data: bytes) -> int:
    """hash.CRC32C, bit by bit over Python ints (small inputs) — independent of the library"""
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        table.append(c)
    c = 0xFFFFFFFF
    for b in data:
        c = table[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def sections(vectors, dim, graph, quant=QUANT_NONE, codes=None, pq_scales=None, pq_offsets=None, pq_codebooks=None, int4_min=None,
             int4_diff=None, ids=None, metadata=None, metadata_index=None) -> dict:
    """The body's sections in file order, name -> bytes (absent: b"")."""
    vectors = np.ascontiguousarray(vectors, "<f4").reshape(-1, dim)
    rows = vectors.shape[0]
    out = {"vectors": vectors.tobytes(),                                                   # :697-704
           "graph": np.ascontiguousarray(graph, "<u4").reshape(rows, -1).tobytes()}        # :706-724
    out["codes"] = b"" if quant == QUANT_NONE else np.ascontiguousarray(codes, np.uint8).tobytes()   # :727-739
    if quant == QUANT_PQ:                                                                   # :742-763, no (m, K) in front
        out["params"] = np.ascontiguousarray(pq_scales, "<f4").tobytes() + np.ascontiguousarray(pq_offsets, "<f4").tobytes() + \
            np.ascontiguousarray(pq_codebooks, np.int8).tobytes()
    elif quant == QUANT_INT4:                                                               # :764-775
        out["params"] = int4_params(dim, int4_min, int4_diff)
    else:
        out["params"] = b""
    ids = np.arange(rows, dtype="<u8") if ids is None else np.ascontiguousarray(ids, "<u8")
    out["pk"] = ids.tobytes()                                                               # :778-794
    out["metadata"] = nil_metadata(rows) if metadata is None else bytes(metadata)           # :796-823
    out["metadata_index"] = nil_metadata_index() if metadata_index is None else bytes(metadata_index)   # :825-833
    return out


def image(segment_id, vectors, dim, metric, graph, entry, search_list=100, compression=1, quant=QUANT_NONE, pq_m=0, checksum=crc32c,
          **kw) -> bytes:
    """The bytes Flush writes.  vectors / graph / codes / ids / metadata: in the REORDERED row order; kw: sections()' arguments."""
    sec = sections(vectors, dim, graph, quant=quant, **kw)
    rows = len(sec["pk"]) // 8
    r = len(sec["graph"]) // (4 * rows)
    body = b"".join(sec.values())
    at, start = HEADER_SIZE, {}                                                             # :695 bytesWritten
    for name, b in sec.items():
        start[name] = at
        at += len(b)
    head = bytearray(HEADER_SIZE)                                                           # format.go:51-78
    struct.pack_into("<IIQII", head, 0, MAGIC, VERSION, segment_id, rows, dim)
    head[24] = int(metric)
    struct.pack_into("<III", head, 25, r, search_list, entry)
    head[37] = quant
    if quant == QUANT_PQ:                                                                   # writer.go:678-681
        struct.pack_into("<HH", head, 38, pq_m, 256)
    head[42] = compression
    pq_codes = start["codes"] if quant in (QUANT_PQ, QUANT_INT4) else 0                     # :728-732: set inside their branches only
    bq_codes = start["codes"] if quant == QUANT_RABITQ else 0
    codebook = start["params"] if sec["params"] else 0                                      # :743, :766
    struct.pack_into("<9Q", head, 48, start["vectors"], start["graph"], pq_codes, bq_codes, codebook, start["pk"], start["metadata"],
                     0, start["metadata_index"])                                            # BlockStatsOffset: never set
    struct.pack_into("<I", head, 120, checksum(body))
    return bytes(head) + body


def parse_header(buf: bytes) -> dict:
    """format.go:80-119 DecodeHeader"""
    assert len(buf) >= HEADER_SIZE, "buffer too small for header"
    magic, version, seg, rows, dim = struct.unpack_from("<IIQII", buf, 0)
    assert magic == MAGIC and version == VERSION
    r, l, entry = struct.unpack_from("<III", buf, 25)
    m, k = struct.unpack_from("<HH", buf, 38)
    out = {"segment_id": seg, "rows": rows, "dim": dim, "metric": buf[24], "max_degree": r, "search_list_size": l, "entrypoint": entry,
           "quant": buf[37], "pq_m": m, "pq_k": k, "compression": buf[42], "checksum": struct.unpack_from("<I", buf, 120)[0]}
    out.update(zip(_OFFSETS, struct.unpack_from("<9Q", buf, 48)))
    return out
