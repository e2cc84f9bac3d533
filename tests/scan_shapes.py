"""How the whole-segment code scans (SQ8, RaBitQ, PQ ADC) cut and deal their 64-row tiles, restated in Python so that a test
can size itself to reach a given trip count and say which kernel it reached.  No GPU.

  scan_slices   vecgo_amd/csrc/vg_scan_slices.hpp (tests/cpp/host_mirror_test.cpp pins the same cases at compile time)
  tile_of       the one-query deal of sq8_scan_kernel, rabitq_scan_kernel and pq_adc_scan_kernel<.., ONCE = true>:
                trip i of workgroup s, wave w scores tile (i * slices + s) * waves + w
  sq8_wide      vg_search_sq8: one query over at least 8 tiles per slice runs the 8-wave workgroup
  int4_plan     vecgo_amd/csrc/vg_int4_plan.hpp (pinned the same way): the kernel and launch shape of a one-query INT4 distance scan
  int4_trips    the tiles a persistent wave of int4_scan_tab_kernel walks: wave w of workgroup b takes tiles b * waves + w,
                + blocks * waves, ...
"""

SQ8_WAVES, SQ8_WIDE_WAVES, RABITQ_WAVES, ADC_WAVES = 4, 8, 4, 8
RABITQ_MQ, SQ8_MQ = 16, 4      # queries per workgroup of the several-query kernels (kRqMq, kSqProbeQ)


def scan_slices(units, tile_groups, cus, wg_per_cu):
    want = ((wg_per_cu * cus + units - 1) // units + 7) // 8 * 8
    most = max(tile_groups // 8 * 8, 8)
    return most if want > most else max(want, 8)


def n_tiles(n):
    return (n + 63) // 64


def tile_of(trip, s, wave, slices, waves):
    return (trip * slices + s) * waves + wave


def trips(tiles, slices, waves):
    """(largest, smallest) number of tiles a wave of the deal scores: wave j of the slices * waves dealt waves takes tiles
    j, j + step, j + 2 step, ... below `tiles`"""
    step = slices * waves
    return (tiles + step - 1) // step, tiles // step


INT4_PAIR_WAVES, INT4_TAB_WAVES, INT4_TAB_STRIDE, INT4_TAB_MAX_DIM, INT4_TAB_LDS, INT4_SMALL_GRID = 4, 12, 144, 1024, 160 * 1024, 2


def int4_plan(dim, codes_aligned16, n, cus, small_grid=False):
    """(kernel, waves, blocks, dynamic LDS bytes) of vg::int4_scan_plan; kernel is "tab", "pair128", "pair_tail" or "row" """
    tiles = n_tiles(n)
    if dim % 64 or not codes_aligned16:
        return "row", 4, (n + 255) // 256, 0
    if dim % 256 == 0 and dim <= INT4_TAB_MAX_DIM:
        waves = min(INT4_TAB_WAVES, (INT4_TAB_LDS - dim * 64) // (64 * INT4_TAB_STRIDE))
        cap = INT4_SMALL_GRID if small_grid else max(cus, 1)
        return "tab", waves, min((tiles + waves - 1) // waves, cap), dim * 64 + waves * 64 * INT4_TAB_STRIDE
    return ("pair128" if (dim // 2) % 128 == 0 else "pair_tail"), INT4_PAIR_WAVES, (tiles + INT4_PAIR_WAVES - 1) // INT4_PAIR_WAVES, 0


def int4_trips(n, blocks, waves):
    """(largest, smallest) number of tiles a wave of the table scan walks (0: the wave returns after the barrier)"""
    return trips(n_tiles(n), blocks, waves)


def slices_for(n, cus, wg_per_cu, tile_group=1, units=1):
    """the slices of a scan over n rows: tile_group tiles make one of scan_slices' tile groups (the ADC scan counts its tiles in
    workgroup-iterations of 8 waves)"""
    return scan_slices(units, (n_tiles(n) + tile_group - 1) // tile_group, cus, wg_per_cu)


def sq8_wide(nq, tiles, slices):
    return nq == 1 and tiles >= 8 * slices


def rows_for(trips_wanted, cus, wg_per_cu, waves, tile_group=1):
    """A row count at which a one-query scan's busiest waves make exactly trips_wanted trips, the others one fewer, and the last
    tile is ragged (n % 64 neither 0 nor 63): trips_wanted - 1 whole rounds of the deal and about a seventh more (9375 rows per
    128 tiles of those rounds: 300 000 rows per 4096 tiles), then up to the next ragged count."""
    assert 2 <= trips_wanted <= 7
    step = scan_slices(1, 1 << 40, cus, wg_per_cu) * waves          # (enough tiles: the slices the CUs ask for)
    n = (trips_wanted - 1) * step * 9375 // 128 + 1
    while n % 64 in (0, 63):
        n += 1
    slices = slices_for(n, cus, wg_per_cu, tile_group)
    if slices * waves != step or trips(n_tiles(n), slices, waves) != (trips_wanted, trips_wanted - 1):
        raise ValueError(f"no {trips_wanted}-trip size for {cus} CUs x {wg_per_cu}, {waves} waves: {n} rows give "
                         f"{slices} slices, trips {trips(n_tiles(n), slices, waves)}")
    return n
