"""tests/scan_shapes.py against the cases tests/cpp/host_mirror_test.cpp static_asserts for vg::scan_slices (the header and its
Python restatement must not drift apart), the same for vg::int4_scan_plan, and the dealt mapping on cases small enough to count by hand."""
import pytest

from tests import scan_shapes as sh

# (units, tile_groups, cus, wg_per_cu) -> slices: the same lines as host_mirror_test.cpp
SLICE_CASES = [
    ((1, 15625, 256, 4), 1024),
    ((3, 15625, 256, 4), 344),
    ((256, 15625, 256, 4), 8),
    ((1, 100, 256, 4), 96),
    ((1, 5, 256, 4), 8),
    ((1, 1954, 256, 1), 256),
    ((1024, 1954, 256, 1), 8),
    # the sizes tests/test_gpu_scan_trips.py runs on 256 CUs
    ((1, 4688, 256, 4), 1024),      # 300 001 rows: SQ8 4 waves, RaBitQ generic
    ((1, 586, 256, 1), 256),        # 300 001 rows in groups of 8 tiles: ADC
    ((1, 9376, 256, 4), 1024),      # 600 001 rows: RaBitQ ring, SQ8 8 waves
    ((65, 313, 256, 4), 16),        # 20 000 rows, 1030 RaBitQ queries in blocks of 16
    ((150, 313, 256, 4), 8),        # 20 000 rows, 600 SQ8 queries in groups of 4
]


@pytest.mark.parametrize("args,slices", SLICE_CASES)
def test_scan_slices_matches_the_header(args, slices):
    assert sh.scan_slices(*args) == slices


def test_tile_of_and_trips_by_hand():
    # 2 slices of 4 waves: 8 dealt waves; trip 0 is tiles 0..7 in (slice, wave) order, trip 1 tiles 8..15
    assert [sh.tile_of(0, s, w, 2, 4) for s in range(2) for w in range(4)] == list(range(8))
    assert sh.tile_of(1, 0, 0, 2, 4) == 8 and sh.tile_of(1, 1, 3, 2, 4) == 15 and sh.tile_of(2, 1, 0, 2, 4) == 20
    assert sh.trips(8, 2, 4) == (1, 1)          # every wave one tile
    assert sh.trips(9, 2, 4) == (2, 1)          # tile 8: a second trip for slice 0, wave 0 alone
    assert sh.trips(16, 2, 4) == (2, 2)
    assert sh.trips(17, 2, 4) == (3, 2)
    assert sh.trips(5, 2, 4) == (1, 0)          # fewer tiles than waves
    # every tile is dealt exactly once
    tiles, slices, waves = 37, 8, 4
    most, _ = sh.trips(tiles, slices, waves)
    dealt = sorted(t for i in range(most) for s in range(slices) for w in range(waves)
                   if (t := sh.tile_of(i, s, w, slices, waves)) < tiles)
    assert dealt == list(range(tiles))


def test_sq8_width_rule():
    assert not sh.sq8_wide(1, 8191, 1024) and sh.sq8_wide(1, 8192, 1024) and not sh.sq8_wide(2, 9376, 1024)


@pytest.mark.parametrize("want,wg_per_cu,waves,tile_group,n,tiles,slices", [
    (2, 4, 4, 1, 300_001, 4688, 1024),      # SQ8 4 waves, RaBitQ generic: 2 / 1 trips
    (3, 1, 8, 8, 300_001, 4688, 256),       # ADC: 3 / 2 trips
    (3, 4, 4, 1, 600_001, 9376, 1024),      # RaBitQ ring: 3 / 2 trips
    (2, 4, 8, 1, 600_001, 9376, 1024),      # SQ8 8 waves: 2 / 1 trips
])
def test_rows_for_on_256_cus(want, wg_per_cu, waves, tile_group, n, tiles, slices):
    assert sh.rows_for(want, 256, wg_per_cu, waves, tile_group) == n
    assert sh.n_tiles(n) == tiles and sh.slices_for(n, 256, wg_per_cu, tile_group) == slices
    assert sh.trips(tiles, slices, waves) == (want, want - 1)
    assert n % 64 not in (0, 63)
    if wg_per_cu == 4:                         # the SQ8 / RaBitQ slices: 600 001 rows reach SQ8's 8-wave workgroup
        assert sh.sq8_wide(1, tiles, slices) == (n == 600_001)


# (dim, codes 16-byte aligned, rows, CUs, VG_INT4_SMALL_GRID) -> (kernel, waves, workgroups, dynamic LDS bytes): the same lines as
# the I4_PLAN static_asserts of host_mirror_test.cpp for vg::int4_scan_plan
M = 1_000_000
INT4_PLAN_CASES = [
    ((64, True, M, 256, False), ("pair_tail", 4, 3907, 0)), ((64, False, M, 256, False), ("row", 4, 3907, 0)),
    ((128, True, M, 256, False), ("pair_tail", 4, 3907, 0)), ((128, False, M, 256, False), ("row", 4, 3907, 0)),
    ((192, True, M, 256, False), ("pair_tail", 4, 3907, 0)), ((192, False, M, 256, False), ("row", 4, 3907, 0)),
    ((320, True, M, 256, False), ("pair_tail", 4, 3907, 0)), ((320, False, M, 256, False), ("row", 4, 3907, 0)),
    ((1088, True, M, 256, False), ("pair_tail", 4, 3907, 0)), ((1088, False, M, 256, False), ("row", 4, 3907, 0)),
    ((1280, True, M, 256, False), ("pair128", 4, 3907, 0)), ((1280, False, M, 256, False), ("row", 4, 3907, 0)),
    ((1536, True, M, 256, False), ("pair128", 4, 3907, 0)), ((1536, False, M, 256, False), ("row", 4, 3907, 0)),
    ((3072, True, M, 256, False), ("pair128", 4, 3907, 0)), ((3072, False, M, 256, False), ("row", 4, 3907, 0)),
    ((1536, True, 5, 256, True), ("pair128", 4, 1, 0)), ((1536, True, 833, 256, False), ("pair128", 4, 4, 0)),
    ((2056, True, M, 256, False), ("row", 4, 3907, 0)), ((2056, False, M, 256, False), ("row", 4, 3907, 0)),
    ((2056, True, 130, 256, True), ("row", 4, 1, 0)), ((95, True, 130, 256, False), ("row", 4, 1, 0)),
    ((256, True, M, 256, False), ("tab", 12, 256, 126976)), ((256, False, M, 256, False), ("row", 4, 3907, 0)),
    ((768, True, M, 256, False), ("tab", 12, 256, 159744)), ((768, False, M, 256, False), ("row", 4, 3907, 0)),
    ((1024, True, M, 256, False), ("tab", 10, 256, 157696)), ((1024, False, M, 256, False), ("row", 4, 3907, 0)),
] + [case for dim, waves, lds, few in ((256, 12, 126976, 4), (512, 12, 143360, 4), (768, 12, 159744, 4), (1024, 10, 157696, 5)) for case in (
    ((dim, True, M, 304, False), ("tab", waves, 304, lds)),
    ((dim, True, M, 256, True), ("tab", waves, 2, lds)),
    ((dim, True, 3000, 256, False), ("tab", waves, few, lds)),
    ((dim, True, 3000, 256, True), ("tab", waves, 2, lds)),
    ((dim, True, 65, 256, True), ("tab", waves, 1, lds)),
    ((dim, True, 1, 0, False), ("tab", waves, 1, lds)))]


@pytest.mark.parametrize("args,plan", INT4_PLAN_CASES)
def test_int4_plan_matches_the_header(args, plan):
    assert sh.int4_plan(*args) == plan


def test_int4_plan_cases_are_the_static_asserts():
    """every I4_PLAN line of host_mirror_test.cpp is a case above and the other way round: neither list can grow alone"""
    import pathlib
    import re
    src = (pathlib.Path(__file__).resolve().parent / "cpp" / "host_mirror_test.cpp").read_text()
    names = {"kI4Tab": "tab", "kI4Pair128": "pair128", "kI4PairTail": "pair_tail", "kI4Row": "row"}
    lines = re.findall(r"^I4_PLAN\((\d+), (true|false), (\d+), (\d+), (true|false), (\w+), (\d+), (\d+), (\d+)\);", src, flags=re.M)
    asserted = {((int(d), a == "true", int(n), int(c), h == "true"), (names[k], int(w), int(b), int(l))) for d, a, n, c, h, k, w, b, l in lines}
    assert asserted == set(INT4_PLAN_CASES) and len(lines) == len(INT4_PLAN_CASES)


def test_int4_scan_plan_is_exported_and_bound():
    import ctypes as C

    import vecgo_amd
    from vecgo_amd import _lib
    lib = _lib.load()
    assert "vg_int4_scan_plan" in _lib.declared_symbols() and hasattr(lib, "vg_int4_scan_plan")
    assert lib.vg_int4_scan_plan(None, C.c_int64(1), 1, None) == -1           # a NULL quantizer is a status, not a crash
    assert callable(vecgo_amd.Int4Quantizer.scan_plan) and vecgo_amd.Int4Quantizer.SCAN_KERNELS == ("tab", "pair128", "pair_tail", "row")
    assert lib.vg_debug_set_hook(b"VG_INT4_SMALL_GRID", 0) == 0               # the hook's name is known


def test_int4_trips_by_hand():
    # 2 workgroups of 12 waves: 24 persistent waves, wave j walks tiles j, j + 24, ...
    assert sh.int4_trips(64 * 24, 2, 12) == (1, 1) and sh.int4_trips(64 * 24 + 1, 2, 12) == (2, 1)
    assert sh.int4_trips(64 * 72, 2, 12) == (3, 3) and sh.int4_trips(4700, 2, 12) == (4, 3) and sh.int4_trips(3900, 2, 10) == (4, 3)
    assert sh.int4_trips(5 * 64, 1, 12) == (1, 0)                           # idle waves
    assert sh.tile_of(3, 1, 11, 2, 12) == 95                                # trip 3 of the last wave: tile 3 * 24 + 12 + 11


@pytest.mark.parametrize("cus", [8, 64, 120, 228, 256, 304])
def test_rows_for_holds_its_properties_on_other_cu_counts(cus):
    for want, wg_per_cu, waves, tile_group in ((2, 4, 4, 1), (3, 4, 4, 1), (2, 4, 8, 1), (3, 1, 8, 8)):
        n = sh.rows_for(want, cus, wg_per_cu, waves, tile_group)
        slices = sh.slices_for(n, cus, wg_per_cu, tile_group)
        assert sh.trips(sh.n_tiles(n), slices, waves) == (want, want - 1) and n % 64 not in (0, 63)
