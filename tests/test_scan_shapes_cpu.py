"""tests/scan_shapes.py against the cases tests/cpp/host_mirror_test.cpp static_asserts for vg::scan_slices (the header and its
Python restatement must not drift apart), and the dealt mapping on cases small enough to count by hand."""
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


@pytest.mark.parametrize("cus", [8, 64, 120, 228, 256, 304])
def test_rows_for_holds_its_properties_on_other_cu_counts(cus):
    for want, wg_per_cu, waves, tile_group in ((2, 4, 4, 1), (3, 4, 4, 1), (2, 4, 8, 1), (3, 1, 8, 8)):
        n = sh.rows_for(want, cus, wg_per_cu, waves, tile_group)
        slices = sh.slices_for(n, cus, wg_per_cu, tile_group)
        assert sh.trips(sh.n_tiles(n), slices, waves) == (want, want - 1) and n % 64 not in (0, 63)
