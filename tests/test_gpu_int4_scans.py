"""Every kernel vg_int4_l2_distance_batch can pick (vecgo_amd/csrc/vg_int4_plan.hpp), at its seams: EVERY row's score bits against
the oracle, for both summation orders (l2_distance_batch: the batch kernel's order; l2_distance: the lookup-table order, row by row).

Each case first asserts, from vg_int4_scan_plan, the kernel and body it is about — "tab" (int4_scan_tab_kernel: persistent waves,
counted LDS waits), "pair128" / "pair_tail" (the two bodies of int4_scan_kernel), "row" (a lane per row) — and that the Python
restatement (tests/scan_shapes.py) agrees; cases about the persistent walk also assert how many tiles a wave walks.  Under the
test hook VG_INT4_SMALL_GRID the table scan runs on 2 workgroups, so a few thousand rows walk every wave over 3 or 4 tiles on any
device.

Inputs are built so that a wrong carry or a wrong order changes bits: min ~ N(0, 0.5) and diff log-uniform over 2^-4 .. 2^4 per
dimension (the order of additions and the dimension a byte is decoded under show in the low bits), the query a decoded random code
plus noise of half a code step, the codes random bytes with planted rows — all 0x00, 0xFF, 0xF0, 0x0F (nibble order), the query's
own code, and for every 16-byte block of the row a row of 0x77 that differs in that block alone (a block scored under the wrong
dimensions or into the wrong accumulator shows in that row) — repeated in the first tile, in the last (ragged) tile and, for a
walk, in a tile of every trip of one of the busiest waves."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import devbuf as db
from tests import hooks
from tests import scan_shapes as sh

pytestmark = pytest.mark.gpu


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


@pytest.fixture(scope="module")
def cus(ctx):
    return ctx.device_info()["compute_units"]


def quantizers(vg, ctx, rng, dim):
    mn = (rng.standard_normal(dim) * 0.5).astype(np.float32)
    df = np.exp2(rng.uniform(-4.0, 4.0, dim)).astype(np.float32)
    iq = vg.Int4Quantizer(ctx, dim); iq.set_params(mn, df)
    ref = o.Int4Quantizer(dim); ref.set_params(mn, df)
    return iq, ref


def planted_rows(rng, cq, cb):
    """the rows to plant: four constant rows, the query's code, and one row per 16-byte block (0x77 outside the block, bytes that
    all differ from 0x77 inside it)"""
    rows = [np.full(cb, v, np.uint8) for v in (0x00, 0xFF, 0xF0, 0x0F)] + [cq.copy()]
    for b0 in range(0, cb, 16):
        r = np.full(cb, 0x77, np.uint8)
        w = min(16, cb - b0)
        r[b0:b0 + w] = (0x77 + rng.integers(1, 256, w)) & 0xFF
        rows.append(r)
    return rows


def build(vg, ctx, dim, n, seed, extra_tiles=()):
    """quantizers, query and n rows of codes with the planted rows in the first tile, in `extra_tiles` and in the last tile.  A
    tile takes the planted rows from the first on (more than 64 of them, dim > 1888: each site starts 64 further on, so whole
    tiles between them hold them all)."""
    rng = np.random.default_rng(seed)
    iq, ref = quantizers(vg, ctx, rng, dim)
    cb = (dim + 1) // 2
    cq = rng.integers(0, 256, cb, dtype=np.uint8)
    if dim & 1:
        cq[-1] &= 0xF0
    step = ref.diff / np.float32(15.0)
    q = (ref.decode(cq) + rng.standard_normal(dim).astype(np.float32) * np.float32(0.5) * step).astype(np.float32)
    codes = rng.integers(0, 256, (n, cb), dtype=np.uint8)
    rows = planted_rows(rng, cq, cb)
    tiles = sh.n_tiles(n)
    sites = list(dict.fromkeys([0, *extra_tiles, tiles - 1]))
    assert all(0 <= t < tiles for t in sites)
    placed = set()
    for s, t in enumerate(sites):
        first = (s * 64) % len(rows) if len(rows) > 64 else 0
        for i, row in enumerate(range(t * 64, min(n, t * 64 + 64))):
            if i >= len(rows) and len(rows) <= 64:
                break
            codes[row] = rows[(first + i) % len(rows)]
            placed.add((first + i) % len(rows))
    whole = sum(1 for t in sites if t * 64 + 64 <= n)
    if whole * 64 >= len(rows):
        assert len(placed) == len(rows)                     # every block's row is somewhere
    return iq, ref, q, codes


def where(got, want):
    bad = np.flatnonzero(bits(got) != bits(want))
    return f"{bad.size} rows differ, first {bad[:8].tolist()} (tiles {sorted(set((bad // 64).tolist()))[:8]})"


def check_both_orders(iq, ref, q, codes, call_codes=None):
    """every row, both orders; call_codes: the buffer the library is given when that is not the host array"""
    given = codes if call_codes is None else call_codes
    got_b, got_p = db.to_host(iq.l2_distance_batch(q, given)), db.to_host(iq.l2_distance(q, given))
    want_b = ref.l2_distance_batch(q, codes)
    want_p = np.array([ref.l2_distance(q, c) for c in codes], np.float32)
    assert got_b.shape == want_b.shape == got_p.shape == want_p.shape == (codes.shape[0],)
    assert np.array_equal(bits(got_b), bits(want_b)), "batch order: " + where(got_b, want_b)
    assert np.array_equal(bits(got_p), bits(want_p)), "table order: " + where(got_p, want_p)
    return got_b, got_p


def assert_plan(iq, dim, n, cus, kernel, aligned=True, small_grid=False):
    plan = iq.scan_plan(n, aligned)
    assert plan["kernel"] == kernel, (dim, n, plan)
    assert (plan["kernel"], plan["waves"], plan["blocks"], plan["lds"]) == sh.int4_plan(dim, aligned, n, cus, small_grid), (dim, n, plan)
    return plan


# ---- int4_scan_kernel, rows of whole 128-byte pieces (dim % 256 == 0 above the table scan's 1024) ----------------------------------
# 5 rows: fewer than the 8 a lane helps to load, every clamp goes to row n - 1; 64 / 65: one whole tile, and one row of a second;
# 64 * 4 * 3 + 64 + 17: three whole workgroups, then one whole tile and a ragged one in the last
@pytest.mark.parametrize("n", [5, 64, 65, 64 * 4 * 3 + 64 + 17])
@pytest.mark.parametrize("dim", [1280, 1536, 2048, 3072])
def test_pair128(vg, ctx, cus, dim, n):
    iq, ref, q, codes = build(vg, ctx, dim, n, 128 * dim + n, extra_tiles=[t for t in (1, 5, 12) if t < sh.n_tiles(n) - 1])
    plan = assert_plan(iq, dim, n, cus, "pair128")
    assert plan["blocks"] == (sh.n_tiles(n) + 3) // 4 and plan["waves"] == 4
    check_both_orders(iq, ref, q, codes)


# ---- int4_scan_kernel, a last piece of 32, 64 or 96 bytes --------------------------------------------------------------------------
# 128, 384, 896: a 64-byte tail after 0, 1 and 3 whole pieces; 448, 960: a 96-byte tail after 1 and 3; 1088, 1216, 1984: four or
# more pieces and a tail of 32, 96 and 96 bytes
@pytest.mark.parametrize("n", [1, 63, 64, 321])
@pytest.mark.parametrize("dim", [128, 384, 896, 448, 960, 1088, 1216, 1984])
def test_pair_tail(vg, ctx, cus, dim, n):
    iq, ref, q, codes = build(vg, ctx, dim, n, 64 * dim + n, extra_tiles=[t for t in (1, 4) if t < sh.n_tiles(n) - 1])
    assert (dim // 2) % 128 in (32, 64, 96)
    assert_plan(iq, dim, n, cus, "pair_tail")
    check_both_orders(iq, ref, q, codes)


# ---- int4_scan_tab_kernel, as launched ---------------------------------------------------------------------------------------------
# fewer tiles than waves (idle waves return after the barrier), exactly as many, one more (a second workgroup with one live wave);
# ragged by 63, 1 (lim = 0 in `offsets`) and 2
@pytest.mark.parametrize("tiles_over,rem", [(-3, 63), (0, 1), (1, 2)])
@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_tab_few_tiles(vg, ctx, cus, dim, tiles_over, rem):
    waves = sh.int4_plan(dim, True, 1, cus)[1]
    assert waves == (10 if dim == 1024 else 12)
    tiles = waves + tiles_over
    n = (tiles - 1) * 64 + rem
    iq, ref, q, codes = build(vg, ctx, dim, n, 16 * dim + n, extra_tiles=[tiles // 2])
    plan = assert_plan(iq, dim, n, cus, "tab")
    assert plan["waves"] == waves and sh.n_tiles(n) == tiles and n % 64 == rem
    if cus >= 2:
        assert plan["blocks"] == (2 if tiles_over > 0 else 1)
        assert sh.int4_trips(n, plan["blocks"], waves) == ((1, 1) if tiles_over == 0 else (1, 0))
    check_both_orders(iq, ref, q, codes)


# ---- int4_scan_tab_kernel on 2 workgroups: the persistent walk ---------------------------------------------------------------------
def run_tab_walk(vg, ctx, cus, dim, tiles_of, rem, want_trips):
    waves = sh.int4_plan(dim, True, 1, cus, True)[1]
    tiles = tiles_of(waves)
    n = tiles * 64 if rem == 0 else (tiles - 1) * 64 + rem
    most = want_trips[0]
    # the tiles of one of the busiest waves, workgroup 0 wave 0: one per trip
    busy = [sh.tile_of(i, 0, 0, sh.INT4_SMALL_GRID, waves) for i in range(most)]
    iq, ref, q, codes = build(vg, ctx, dim, n, 4 * dim + n, extra_tiles=busy)
    hooks.set_hook("VG_INT4_SMALL_GRID", 1)
    try:
        plan = assert_plan(iq, dim, n, cus, "tab", small_grid=True)
        assert plan["blocks"] == 2 and plan["waves"] == waves == (10 if dim == 1024 else 12)
        assert sh.int4_trips(n, plan["blocks"], plan["waves"]) == want_trips and sh.n_tiles(n) == tiles
        assert busy[-1] < tiles
        got = check_both_orders(iq, ref, q, codes)
    finally:
        hooks.set_hook("VG_INT4_SMALL_GRID", 0)
    unhooked = iq.scan_plan(n)
    assert (unhooked["kernel"], unhooked["waves"], unhooked["lds"]) == (plan["kernel"], plan["waves"], plan["lds"])
    if unhooked["blocks"] > 2:                              # the launch as it is made without the hook: more workgroups, the same bits
        again = (iq.l2_distance_batch(q, codes), iq.l2_distance(q, codes))
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again))
    return n


@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_tab_walk_four_and_three_trips_ragged(vg, ctx, cus, dim):
    """6 * waves + 2 tiles: waves 0 and 1 of workgroup 0 walk 4 tiles, the others 3; the last tile is ragged and is reached as a
    NEXT tile (`von`) by wave 1 in its 4th trip; `tbase` / `vo` carried over three seams"""
    n = run_tab_walk(vg, ctx, cus, dim, lambda w: 6 * w + 2, 37, (4, 3))
    assert n == (3941 if dim == 1024 else 4709)


@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_tab_walk_three_trips_even(vg, ctx, cus, dim):
    """6 * waves whole tiles: every wave walks exactly 3, and requests its last tile again (tnext == tile) while it scores it"""
    run_tab_walk(vg, ctx, cus, dim, lambda w: 6 * w, 0, (3, 3))


@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_tab_walk_single_tile_rerequested(vg, ctx, cus, dim):
    """2 * waves - 1 tiles on 2 workgroups: every live wave walks ONE tile and re-requests it, the last one ragged by 2 rows (its
    re-request is clamped the same way); the last wave of workgroup 1 is idle"""
    run_tab_walk(vg, ctx, cus, dim, lambda w: 2 * w - 1, 2, (1, 0))


# ---- a lane per row ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [256, 1536])
def test_row_kernels_through_alignment_alone(vg, ctx, cus, dim):
    """dim % 64 == 0, the codes 4 bytes past a 16-byte boundary: the lane-per-row kernels, and the bits of the aligned call"""
    import torch
    n = 300
    iq, ref, q, codes = build(vg, ctx, dim, n, 2 * dim + n, extra_tiles=[2])
    view = db.offset_like(codes, 4)
    assert view.data_ptr() % 16 == 4
    assert_plan(iq, dim, n, cus, "row", aligned=False)
    assert_plan(iq, dim, n, cus, "tab" if dim == 256 else "pair128")
    torch.cuda.synchronize()
    skewed = (iq.l2_distance_batch(q, view), iq.l2_distance(q, view))
    torch.cuda.synchronize()
    aligned = check_both_orders(iq, ref, q, codes)
    for s, a in zip(skewed, aligned):
        assert np.array_equal(bits(db.to_host(s)), bits(a)), where(db.to_host(s), a)


# 95: 64-blocks with no 32-block (one 64-block, 31 scalar dimensions, an odd dimension count); 96: one 64-block and one 32-block;
# 2056: a long run of 64-blocks with an 8-wide tail
@pytest.mark.parametrize("dim", [95, 96, 2056])
def test_row_kernels_odd_dimensions(vg, ctx, cus, dim):
    n = 130
    iq, ref, q, codes = build(vg, ctx, dim, n, 3 * dim + n, extra_tiles=[1])
    assert_plan(iq, dim, n, cus, "row")
    check_both_orders(iq, ref, q, codes)


# ---- codec: a second block of dimensions ---------------------------------------------------------------------------------------------
# int4_encode8_kernel / int4_decode8_kernel: 256 threads of 8 dimensions per block — 2056: the second block has ONE live thread,
# 4096: it is full
@pytest.mark.parametrize("dim", [2056, 4096])
def test_codec_second_block_of_dimensions(vg, ctx, dim):
    n = 50
    rng = np.random.default_rng(dim)
    iq, ref = quantizers(vg, ctx, rng, dim)
    x = (ref.min + ref.diff * rng.uniform(-0.3, 1.3, (n, dim)).astype(np.float32)).astype(np.float32)
    x[0], x[1] = ref.min - 9 * ref.diff, ref.min + 9 * ref.diff            # all below, all above the range
    x[2, -8:] = ref.min[-8:] + 40 * ref.diff[-8:]                         # the last thread's dimensions above, its neighbours' below
    x[2, -16:-8] = ref.min[-16:-8] - 40 * ref.diff[-16:-8]
    want = ref.encode_batch(x)
    assert want[0].max() == 0x00 and want[1].min() == 0xFF and want[2, -4:].min() == 0xFF and want[2, -8:-4].max() == 0x00
    codes = iq.encode(x)
    assert codes.shape == (n, dim // 2) and np.array_equal(codes, want), np.argwhere(codes != want)[:8]
    every = np.vstack([want, rng.integers(0, 256, (n, dim // 2), dtype=np.uint8)])
    got = iq.decode(every)
    ref_dec = np.stack([ref.decode(c) for c in every])
    assert got.shape == (2 * n, dim) and np.array_equal(bits(got), bits(ref_dec)), np.argwhere(bits(got) != bits(ref_dec))[:8]
