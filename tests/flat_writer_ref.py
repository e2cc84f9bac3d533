"""flat.Writer.Flush restated in numpy for the tests of vg_flat_build / vg_segment_write_flat: the regrouping of the rows by
partition (internal/segment/flat/writer.go:114-165) and the file image (:312-470, header fields flat/format.go:28-56, encoded
as :112-133).  Written from the reference, section by section; unlike tests/segfile.py it pads nothing between sections,
because the reference writer does not."""
from __future__ import annotations

import struct

import numpy as np

HEADER_SIZE = 152          # format.go:110
MAGIC, VERSION = 0x56454331, 1   # format.go:12-13
BLOCK_SIZE = 1024          # format.go:14
QUANT_NONE, QUANT_SQ8, QUANT_PQ = 0, 1, 2   # format.go:22-26

_FIELDS = ("centroid_off", "part_off_off", "quant_off", "codes_off", "vector_off", "pk_off", "metadata_off", "block_stats_off")


def group(assign, k):
    """writer.go:114-165 from the assignments on: counts, starts, the fill loop, the k + 1 offsets.
    Returns (perm, inv_perm, part_offsets): row `new` of the regrouped arrays is old row perm[new]."""
    assign = np.asarray(assign, np.int64)
    n = assign.size
    counts = np.zeros(k, np.int64)
    for p in assign:                      # :117-125 partitionCounts[p]++
        counts[p] += 1
    starts = np.zeros(k, np.int64)
    current = 0
    for i in range(k):                    # :133-138
        starts[i] = current
        current += counts[i]
    offsets = starts.copy()               # :141-142 currentOffsets
    perm = np.zeros(n, np.uint32)
    inv = np.zeros(n, np.uint32)
    for i in range(n):                    # :144-153: row i goes to currentOffsets[p]++
        p = assign[i]
        idx = offsets[p]
        perm[idx] = i
        inv[i] = idx
        offsets[p] += 1
    part_off = np.zeros(k + 1, np.uint32)  # :161-165
    part_off[:k] = starts
    part_off[k] = n
    return perm, inv, part_off


def uvarint(v: int) -> bytes:
    """encoding/binary.AppendUvarint"""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def nil_metadata(rows: int) -> bytes:
    """writer.go:230-292 with every w.metadata[j] nil: rows + 1 zero offsets, an empty blob; nothing at all for rows == 0"""
    return b"" if rows == 0 else bytes(4 * (rows + 1))


def nil_block_stats(rows: int) -> bytes:
    """writer.go:294-307: uvarint(number of blocks), then per block uvarint(len(b)) + b, with b = BlockStats.MarshalBinary of an
    empty field map = uvarint(0) (format.go:58-71)"""
    blocks = (rows + BLOCK_SIZE - 1) // BLOCK_SIZE
    return uvarint(blocks) + (uvarint(1) + uvarint(0)) * blocks


def crc32c(data: bytes) -> int:
    """hash.CRC32C, table-driven over numpy-free Python ints (small inputs) — independent of the library"""
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


def image(segment_id, vectors, dim, metric, centroids=None, part_offsets=None, quant=QUANT_NONE, sq_mins=None, sq_maxs=None,
          pq_m=0, pq_scales=None, pq_offsets=None, pq_codebooks=None, codes=None, ids=None, metadata=None, block_stats=None,
          checksum=crc32c) -> bytes:
    """The bytes Flush writes (:312-470).  vectors: the REGROUPED rows; ids / metadata / block_stats None: 0 .. rows-1 and the
    nil-document sections."""
    vectors = np.ascontiguousarray(vectors, "<f4").reshape(-1, dim)
    rows = vectors.shape[0]
    k = 0 if centroids is None else np.asarray(centroids).reshape(-1, dim).shape[0]
    sec_cent = b"" if k == 0 else np.ascontiguousarray(centroids, "<f4").tobytes()          # :378-382
    sec_poff = b"" if k == 0 else np.ascontiguousarray(part_offsets, "<u4").tobytes()       # :385-389
    if quant == QUANT_SQ8 and rows:                                                          # :392-402
        sec_quant = np.ascontiguousarray(sq_mins, "<f4").tobytes() + np.ascontiguousarray(sq_maxs, "<f4").tobytes()
    elif quant == QUANT_PQ and rows:                                                         # :403-430
        sec_quant = struct.pack("<II", pq_m, 256) + np.ascontiguousarray(pq_scales, "<f4").tobytes() + \
            np.ascontiguousarray(pq_offsets, "<f4").tobytes() + np.ascontiguousarray(pq_codebooks, np.int8).tobytes()
    else:
        sec_quant = b""
    sec_codes = b"" if codes is None else np.ascontiguousarray(codes, np.uint8).tobytes()   # :433-437
    sec_vec = vectors.tobytes()                                                              # :440-444
    ids = np.arange(rows, dtype="<u8") if ids is None else np.ascontiguousarray(ids, "<u8")
    sec_pk = ids.tobytes()                                                                   # :327-333, :447-451
    sec_md = nil_metadata(rows) if metadata is None else bytes(metadata)                     # :454-463
    sec_bs = nil_block_stats(rows) if block_stats is None else bytes(block_stats)            # :466-470
    body = sec_cent + sec_poff + sec_quant + sec_codes + sec_vec + sec_pk + sec_md + sec_bs
    offs, at = [], HEADER_SIZE                                                               # :335-345 running positions
    for sec in (sec_cent, sec_poff, sec_quant, sec_codes, sec_vec, sec_pk, sec_md, sec_bs):
        offs.append(at)
        at += len(sec)
    head = bytearray(HEADER_SIZE)                                                            # format.go:112-133
    struct.pack_into("<IIQII", head, 0, MAGIC, VERSION, segment_id, rows, dim)
    head[24] = int(metric)
    struct.pack_into("<I", head, 28, k)
    head[32] = quant
    struct.pack_into("<8Q", head, 40, *offs)
    struct.pack_into("<I", head, 104, checksum(body))
    return bytes(head) + body


def parse_header(buf: bytes) -> dict:
    """format.go:135-165 DecodeHeader"""
    assert len(buf) >= HEADER_SIZE, "buffer too small for header"
    magic, version, seg, rows, dim = struct.unpack_from("<IIQII", buf, 0)
    assert magic == MAGIC and version == VERSION
    out = {"segment_id": seg, "rows": rows, "dim": dim, "metric": buf[24], "num_partitions": struct.unpack_from("<I", buf, 28)[0],
           "quant": buf[32], "checksum": struct.unpack_from("<I", buf, 104)[0]}
    out.update(zip(_FIELDS, struct.unpack_from("<8Q", buf, 40)))
    return out
