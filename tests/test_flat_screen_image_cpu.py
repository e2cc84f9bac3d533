"""The compact hi-only query image of the flat search's screen (flat_split_queries_kernel's second image, k_flat.hip; read by
flat_gemm_big_body under OPS = kBigScreen, vg_flat_gemm.hpp), without a GPU: a numpy model that RESTATES the three maps —

  image:  element (query R of a 256-query tile, k of a 32-element K step) -> byte of the tile's 16 KiB block of that step
  fill:   (piece p, wave w, lane l) -> the 16 LDS bytes one LDS-DMA lane writes, and the 16 source bytes of the block it reads
  read:   (wave, lane, part of the K step, query block b of the part) -> the 16 LDS bytes of one ds_read_b128 lane, and the
          eight elements (query, k .. k + 7) the matrix instruction takes them for

— and checks that they address the same element for every (query, k) of a tile, and that the 16 lanes of every ds_read_b128 pass
(MI355X: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, {32-35, 44-47, 52-59}, {36-43, 48-51, 60-63}) touch 16 different 16-byte bank
groups of the 256-byte bank window, for all four parts and both halves `wr` of the tile."""
import numpy as np

TILE_Q, STEP_K = 256, 32           # queries of a tile, elements of a K step
ROW_BYTES = STEP_K * 2             # bfloat16: 64 bytes per query and step
BLOCK_BYTES = TILE_Q * ROW_BYTES   # 16 KiB
GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
          list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
          list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def swz(row):
    """what a row's granules are XORed with: four 64-byte rows share a 256-byte bank window"""
    return (row >> 2) & 3


def image_byte(row, k):
    """flat_split_queries_kernel: word w = k / 2 of the step's 16 hi words goes to word
    row * 16 + ((w >> 2) ^ swz(row)) * 4 + (w & 3) of the block; the element is the word's low (even k) or high half"""
    w = k >> 1
    return 4 * (row * 16 + (((w >> 2) ^ swz(row)) << 2) + (w & 3)) + 2 * (k & 1)


def fill_bytes(p, wave, lane):
    """stage_a under SCREEN: pass p is the block's half p (8 KiB), thread t = 64 wave + lane moves the 16 bytes at 16 t of it;
    the LDS-DMA destination is the wave's piece (1 KiB at (8 p + wave) KiB of the tile buffer) + 16 lane.  (source, destination)"""
    src = p * 8192 + 16 * (64 * wave + lane)
    dst = (8 * p + wave) * 1024 + 16 * lane
    return src, dst


def read_byte(wave, lane, part, b):
    """read_part under SCREEN: wave (wr = wave >> 2) covers queries 128 wr .., part = phase part & 1 (query blocks 2 (part & 1) + b)
    of operand group j = part >> 1; lane (r = lane & 31, h = lane >> 5) reads granule 2 j + h of its row.
    -> (LDS byte of the tile buffer, query, first k of the eight elements)"""
    wr, r, h, j = wave >> 2, lane & 31, lane >> 5, part >> 1
    lpart0 = r * 16 + ((h ^ ((lane >> 2) & 3)) * 4)              # floats, group 0's, as the kernel keeps it
    floats = wr * 128 * 16 + (lpart0 ^ (8 * j)) + 2 * (part & 1) * 32 * 16 + b * 32 * 16     # group 1: slot ^ 2
    return 4 * floats, wr * 128 + (2 * (part & 1) + b) * 32 + r, 8 * (2 * j + h)


def lds_contents():
    """element (query, k) held by every 2-byte cell of the tile buffer after the two passes of all eight waves"""
    where = {}
    for row in range(TILE_Q):
        for k in range(STEP_K):
            where[image_byte(row, k)] = (row, k)
    assert len(where) == BLOCK_BYTES // 2 and min(where) == 0 and max(where) == BLOCK_BYTES - 2   # the image is a bijection
    lds = {}
    for p in range(2):
        for wave in range(8):
            for lane in range(64):
                src, dst = fill_bytes(p, wave, lane)
                for e in range(8):
                    assert dst + 2 * e not in lds
                    lds[dst + 2 * e] = where[src + 2 * e]
    assert len(lds) == BLOCK_BYTES // 2                             # every cell written exactly once
    return lds


def test_fill_is_lane_linear_whole_pieces():
    """a piece is one contiguous KiB of the block at the wave's piece of the buffer: 16 rows of 64 B, lane l -> row l >> 2, slot l & 3"""
    for p in range(2):
        for wave in range(8):
            for lane in range(64):
                src, dst = fill_bytes(p, wave, lane)
                assert src == dst and dst % 16 == 0
                assert dst // ROW_BYTES == p * 128 + wave * 16 + (lane >> 2) and (dst % ROW_BYTES) // 16 == (lane & 3)


def test_fill_and_read_address_the_same_elements():
    lds = lds_contents()
    seen = np.zeros((TILE_Q, STEP_K), np.int32)
    for wave in (0, 4):                        # wc = 0 of both wr: the other waves of a wr read the same query rows
        for part in range(4):
            for b in range(2):
                for lane in range(64):
                    byte, q, k0 = read_byte(wave, lane, part, b)
                    assert byte % 16 == 0 and 0 <= byte < BLOCK_BYTES
                    for e in range(8):
                        assert lds[byte + 2 * e] == (q, k0 + e), (wave, part, b, lane, e)
                        seen[q, k0 + e] += 1
    assert np.all(seen == 1)                   # every (query, k) of the tile is multiplied exactly once per wave column
    for wave in range(8):                      # ... and every wave reads its wr's rows, whatever its wc
        for part in range(4):
            assert read_byte(wave, 5, part, 1) == read_byte(wave & 4, 5, part, 1)


def test_every_read_pass_touches_16_bank_groups():
    for wave in (0, 4):
        for part in range(4):
            for b in range(2):
                for group in GROUPS:
                    banks = {(read_byte(wave, lane, part, b)[0] % 256) // 16 for lane in group}
                    assert len(banks) == 16, (wave, part, b, group, sorted(banks))


def test_unswizzled_rows_would_conflict():
    """the check above can fail: with granule g in slot g, a pass puts four rows on each of four bank groups"""
    for group in GROUPS:
        banks = {((lane & 31) * ROW_BYTES + 16 * (lane >> 5)) % 256 // 16 for lane in group}
        assert len(banks) == 4
