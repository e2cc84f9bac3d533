"""tests/exact_dims.py against the constants and gates it restates (vg_exact.hpp, vg_search.hpp, k_flat.hip, k_brute.hip, k_probe.hip,
k_graph.hip: a retune of a chunk size or a gate fails here, so the dimensions get revisited), its loop model on cases small enough to
count by hand, and DIMS against the loop classes tests/test_gpu_exact_dims.py is there to reach."""
import pathlib
import re

import pytest

from tests import exact_dims as ed

CSRC = pathlib.Path(__file__).resolve().parents[1] / "vecgo_amd" / "csrc"


def src(name):
    return (CSRC / name).read_text()


def constant(text, pattern):
    found = re.findall(pattern, text, flags=re.M)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_chunk_constants_are_the_headers():
    h = src("vg_exact.hpp")
    assert constant(h, r"^constexpr int kExactChunk = (\d+);") == ed.EXACT_CHUNK
    assert constant(h, r"^constexpr int kExactChunkSmall = (\d+);") == ed.EXACT_CHUNK_SMALL
    assert constant(h, r"^#define VG_QLDS_CHUNK (\d+)$") == ed.QLDS_CHUNK
    assert len(re.findall(r"^constexpr int kExactChunkQ = VG_QLDS_CHUNK;", h, flags=re.M)) == 1
    assert constant(src("k_graph.hip"), r"^constexpr int kHnswLdsEf = (\d+);") == ed.HNSW_LDS_EF
    # nothing in the build overrides the macro
    assert "VG_QLDS_CHUNK" not in src("Makefile")
    # the register forms: float4 (&rr)[16] and `for (int e = 0; e < 16; e++) if (e < nblk)`
    assert len(re.findall(r"const float4 \(&r\w+\)\[(\d+)\]", h)) == 3 and set(re.findall(r"const float4 \(&r\w+\)\[(\d+)\]", h)) == {"16"}
    assert ed.REGS_MAX_BLOCKS == 16 and ed.BLOCK * ed.REGS_MAX_BLOCKS == 1024


def test_loop_order_is_the_headers():
    """both from-memory scorers walk big chunk -> kExactChunkSmall -> singles, the QLDS form with its own big chunk"""
    h = src("vg_exact.hpp")
    for fn in ("exact_pair16", "exact_l2_both16"):
        body = h[h.index(f"void {fn}(") if fn == "exact_l2_both16" else h.index(f"float {fn}("):]
        body = body[:body.index("\n}\n")]
        heads = re.findall(r"for \(; (.*?); e(?: \+= (\w+)|\+\+)\)", body)
        assert heads == [("e + kExactChunkQ <= nblk", "kExactChunkQ"), ("!QLDS && e + kExactChunk <= nblk", "kExactChunk"),
                         ("e + kExactChunkSmall <= nblk", "kExactChunkSmall"), ("e < nblk", "")], (fn, heads)
        assert "if (QLDS) {" in body


def test_gates_are_the_sources():
    thr = re.search(r"inline bool thr_scan_regs\(const vg_index \*idx\)\n\{\n\s*return (.*);\n", src("vg_search.hpp")).group(1)
    assert thr == "idx->dim % 4 == 0 && idx->dim >= 64 && idx->dim <= 1024 && aligned16(idx->d_vectors)"
    flat = re.search(r"const bool scan_small = (.*?);", src("k_flat.hip"), flags=re.S).group(1)
    assert "c.dim % 4 == 0 && c.dim <= 1024 && c.dim >= 64" in flat and "nq <= kScanMaxBatch" in flat and "k <= 64" in flat
    assert constant(src("k_flat.hip"), r"^constexpr int kScanMaxBatch = (\d+);") >= 3      # the GPU test's nq = 1 and 3 take the scan
    brute = re.search(r"const bool mq = (.*?);", src("k_brute.hip")).group(1)
    assert brute == "cnt >= 2 && idx->dim % 4 == 0 && idx->dim <= 1024 && (m0 == nullptr || mask_stride == 0)"
    probe = re.search(r"^\s+grouped_f32 = (.*?);", src("k_probe.hip"), flags=re.S | re.M).group(1)
    assert "group_ok && idx->dim % 4 == 0 && idx->dim <= 1024" in probe
    for dim, regs, mq in ((0, False, True), (4, False, True), (60, False, True), (63, False, False), (64, True, True), (66, False, False),
                          (68, True, True), (1020, True, True), (1023, False, False), (1024, True, True), (1028, False, False),
                          (2048, False, False)):
        assert ed.regs_form(dim) == regs and ed.brute_mq(dim) == mq, dim


def test_loops_by_hand():
    L = ed.loops
    # 768 floats: one chunk of 12 / two of 6, no tail
    assert ed.trips(768, "plain") == (1, 0, 0) and ed.trips(768, "qlds") == (2, 0, 0) and ed.trips(768, "regs") == (0, 0, 12)
    assert ed.trips(1536, "plain") == (2, 0, 0) and ed.trips(1536, "qlds") == (4, 0, 0)
    assert ed.trips(200, "plain") == ed.trips(200, "qlds") == (0, 0, 3)
    # 23 blocks: 12 + 2 x 4 + 3 / 3 x 6 + 4 + 1
    assert ed.trips(1535, "plain") == (1, 2, 3) and ed.trips(1535, "qlds") == (3, 1, 1)
    # 777 = 12 blocks + 9: no 16-wide step, one 8-wide step and a scalar, nine scalars for kPair
    t = L(777, "plain")
    assert (t.blocks, t.tail, t.batch16, t.batch_scalar, t.bounded8, t.bounded_scalar, t.pair_scalar) == (12, 9, 0, 9, 1, 1, 9)
    t = L(660, "qlds")
    assert (t.blocks, t.tail, t.batch16, t.batch_scalar, t.bounded8, t.bounded_scalar, t.pair_scalar) == (10, 20, 1, 4, 2, 4, 20)
    t = L(63, "plain")
    assert tuple(t[:3]) == (0, 0, 0) and (t.batch16, t.batch_scalar, t.bounded8, t.bounded_scalar) == (3, 15, 7, 7)
    with pytest.raises(ValueError):
        L(1088, "regs")
    with pytest.raises(ValueError):
        L(64, "pair")
    # every block is walked exactly once, every tail float exactly once in every mode
    for dim in range(0, 2100):
        for form, chunk in (("plain", ed.EXACT_CHUNK), ("qlds", ed.QLDS_CHUNK)):
            t = L(dim, form)
            assert t.big * chunk + t.four * ed.EXACT_CHUNK_SMALL + t.single == t.blocks == dim // 64
            assert t.four * ed.EXACT_CHUNK_SMALL + t.single < chunk and t.single < ed.EXACT_CHUNK_SMALL
            assert t.blocks * 64 + t.batch16 * 16 + t.batch_scalar == t.blocks * 64 + t.bounded8 * 8 + t.bounded_scalar == dim
            assert t.blocks * 64 + t.pair_scalar == dim and t.batch_scalar < 16 and t.bounded_scalar < 8


# ---- what DIMS has to reach -------------------------------------------------------------------------------------------------------
PLAIN = [(0, 1, 0), (0, 1, 1), (0, 2, 0), (0, 2, 3), (1, 0, 1), (1, 0, 3), (1, 1, 0), (1, 1, 1), (1, 2, 3), (2, 1, 0)]
QLDS = [(0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 0, 3), (1, 1, 0), (1, 1, 1), (2, 1, 1)]
REG_BLOCKS = [4, 5, 8, 9, 10, 15, 16]


def test_dims_cover_the_block_loop_classes():
    assert ed.DIMS == sorted(set(ed.DIMS)) and 12 <= len(ed.DIMS) <= 17
    plain = {ed.trips(d, "plain") for d in ed.DIMS}
    qlds = {ed.trips(d, "qlds") for d in ed.DIMS}
    assert not set(PLAIN) - plain, set(PLAIN) - plain
    assert not set(QLDS) - qlds, set(QLDS) - qlds
    # the register forms take a dim only through their gates: a block count counts where both gates open
    regs = {ed.loops(d, "regs").blocks for d in ed.DIMS if ed.regs_form(d) and ed.brute_mq(d)}
    assert not set(REG_BLOCKS) - regs, set(REG_BLOCKS) - regs


def test_dims_cover_the_dispatch_edges():
    assert 1028 in ed.DIMS and 1024 in ed.DIMS and 60 in ed.DIMS
    assert ed.regs_form(1024) and ed.brute_mq(1024) and not ed.regs_form(1028) and not ed.brute_mq(1028)   # the upper edge of both gates
    assert not ed.regs_form(60) and ed.brute_mq(60)        # the lower edge of the one gate that has one
    assert 1028 % 4 == 0 and 60 % 4 == 0                   # outside by the size alone, not by the alignment rule
    assert ed.loops(1020, "regs").blocks == 15 and ed.loops(1020, "regs").pair_scalar == 60 and 1020 in ed.DIMS


def test_dims_cover_the_tails():
    tails = {d % 64 for d in ed.DIMS}
    assert {0, 4, 63} <= tails
    plain = {d: ed.loops(d, "plain") for d in ed.DIMS}
    assert any(t.batch16 == 1 and t.batch_scalar == 4 for t in plain.values())                    # one tail of 16 + 4
    assert any(d % 2 == 1 and t.blocks >= 7 for d, t in plain.items())                            # rows not 16-byte aligned
    assert any(t.blocks >= 4 and t.bounded8 >= 1 and t.bounded_scalar >= 1 for t in plain.values())
    assert any(t.blocks >= 4 and t.bounded8 >= 1 and t.bounded_scalar == 0 and t.tail for t in plain.values())
    # behind a block, a kPair tail longer than the 36 floats the suite had before
    assert any(ed.brute_mq(d) and t.blocks >= 1 and t.pair_scalar > 36 for d, t in plain.items())
    # the walk tests pick their Inf-query and tombstone dim by this class
    assert [d for d in ed.DIMS if ed.trips(d, "qlds") == (1, 1, 1)] == [767]
