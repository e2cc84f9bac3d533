"""The whole-segment code scans at sizes where a wave makes more than one trip: ids and score BITS against the oracle.

One query deals the tiles round-robin (tests/scan_shapes.py): trip i of workgroup s, wave w scores tile (i * slices + s) * waves
+ w, and each kernel carries state from trip to trip — the SQ8 load ring refilled from the next tile, the RaBitQ d = 768 ring of
tile slots, the m = 96 ADC scan's two tiles in flight — or changes shape with the size (SQ8: workgroups of 8 waves from 8 tiles
per slice up).  A second trip needs more than slices * waves tiles, over 262 144 rows on 256 CUs.  Every case here sizes itself
from the device's CU count, ASSERTS that it reaches the trips and the kernel it is about, and plants its winners (codes next to
the query's own) where a wrong carry would lose them: in a tile of every trip of one of the busiest waves (identical codes: a tie
across trips, ordered by row id), in the last tile of trip 0 and the first of trip 1 (a tie again), in the ragged last tile, and
for 8-wave workgroups under a wave index above 3.  That the planted rows are the oracle's best is asserted from the oracle's
answer alone.  Codes are random bytes (no float rows are encoded), so a case costs the oracle's pass over the segment."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests import scan_shapes as sh

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF


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


def same(got, qi, eid, esc):
    ids, sc = got
    r = eid.size
    assert np.array_equal(ids[qi, :r], eid), (qi, np.flatnonzero(ids[qi, :r] != eid)[:5], ids[qi, :8], eid[:8])
    assert np.array_equal(bits(sc[qi, :r]), bits(esc)), (qi, np.flatnonzero(bits(sc[qi, :r]) != bits(esc))[:5])
    assert np.all(ids[qi, r:] == PAD)


def launches(ctx, names, call):
    """call() with the context's launch records on: its result and how often each of `names` was launched"""
    ctx.profile_enable(True)
    try:
        for nm in names:
            ctx.profile_read(nm)
        out = call()
        return out, [ctx.profile_read(nm)[0] for nm in names]
    finally:
        ctx.profile_enable(False)


def dealt_plan(n, slices, waves, want_trips, tie_run=0):
    """The preconditions of a dealt case, then where its winners go: [(row, level)] — rows of one level get identical codes (equal
    scores), a lower level is a better score — and the rows of one long run of ties spread over all trips."""
    tiles, step = sh.n_tiles(n), slices * waves
    assert sh.trips(tiles, slices, waves) == (want_trips, want_trips - 1), (n, slices, waves, sh.trips(tiles, slices, waves))
    assert n % 64 not in (0, 63)
    w = waves - 3                                           # wave 1 of 4, wave 5 of 8
    busy = [sh.tile_of(i, 0, w, slices, waves) for i in range(want_trips)]
    assert busy[-1] < tiles - 1 and (waves == 4 or w >= 4)
    plan = [(t * 64 + 7 + i, 1) for i, t in enumerate(busy)]                    # every trip of one busiest wave, one tie
    plan += [((step - 1) * 64 + 63, 2), (step * 64, 2)]                         # last tile of trip 0 = first tile of trip 1
    plan += [(n - 1, 0), (3, 4)]                                                # the segment's last row (the very best); tile 0
    if (tiles - 1) * 64 != n - 1:
        plan.append(((tiles - 1) * 64, 3))                                      # the ragged tile's first row
    run = []
    for j in range(tie_run):
        s = (8 + 3 * j) % slices
        t = sh.tile_of(j % want_trips, s, j % waves, slices, waves)
        if t >= tiles - 1:
            t = sh.tile_of(j % want_trips - 1, s, j % waves, slices, waves)
        run.append(t * 64 + (5 * j) % 64)
    rows = [r for r, _ in plan] + run
    assert len(set(rows)) == len(rows) and max(rows) == n - 1
    if tie_run:
        assert {r // 64 // step for r in run} == set(range(want_trips))
    return plan, run


RUN_LEVEL = 5


def plant(codes, near, plan, run):
    for row, level in plan:
        codes[row] = near(level)
    if run:
        codes[run] = near(RUN_LEVEL)
    return sorted([r for r, _ in plan] + run)


def spread(level, dim):
    return np.unique(np.linspace(0, dim - 1, level).astype(np.int64)) if level else np.zeros(0, np.int64)


# ---- SQ8 ------------------------------------------------------------------------------------------------------------------------
def sq8_quantizer(vg, ctx, rng, dim):
    mins = (rng.standard_normal(dim) - 4).astype(np.float32)
    maxs = (mins + 8 + rng.random(dim)).astype(np.float32)
    sq = vg.ScalarQuantizer(ctx, dim)
    sq.set_bounds(mins, maxs)
    ref = o.ScalarQuantizer(dim)
    ref.mins, ref.inv_scales = mins, np.ascontiguousarray(sq.params()[3])
    ref.trained = True
    return sq, ref


def sq8_query(rng, ref, dim, metric):
    """a query and the code that scores best against it: L2 — the query IS a decoded code; Dot — the code of the largest
    q . x^ (255 where q_j * invScale_j > 0, else 0)"""
    if metric == 0:
        cq = rng.integers(0, 256, dim, dtype=np.uint8)
        return (ref.mins + cq.astype(np.float32) * ref.inv_scales).astype(np.float32), cq
    q = rng.standard_normal(dim).astype(np.float32)
    return q, np.where(q * ref.inv_scales > 0, 255, 0).astype(np.uint8)


def sq8_near(cq):
    def near(level):                                        # `level` codes one step off, spread over the row's groups and its tail
        c = cq.copy()
        p = spread(level, c.size)
        c[p] = np.where(c[p] > 127, c[p] - 1, c[p] + 1)
        return c
    return near


def sq8_oracle(ref, codes, n, dim, metric):
    if metric == 0:
        return lambda q, k: o.flat_search_sq8(ref, codes, q, k)
    seg = o.FlatSegment(np.zeros((n, dim), np.float32), dim, metric=metric, sq=ref, codes=codes)   # (the SQ8 branch reads no rows)
    return lambda q, k: seg.search(q, k)


def run_sq8_dealt(vg, ctx, cus, dim, metric, waves, k, tie_run=0):
    n = sh.rows_for(2, cus, 4, waves)
    slices = sh.slices_for(n, cus, 4)
    assert sh.sq8_wide(1, sh.n_tiles(n), slices) == (waves == sh.SQ8_WIDE_WAVES)
    plan, run = dealt_plan(n, slices, waves, 2, tie_run)
    rng = np.random.default_rng(1000 * dim + 10 * waves + metric)
    sq, ref = sq8_quantizer(vg, ctx, rng, dim)
    q, cq = sq8_query(rng, ref, dim, metric)
    codes = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    planted = plant(codes, sq8_near(cq), plan, run)
    eid, esc = sq8_oracle(ref, codes, n, dim, metric)(q, k)
    assert eid.size == k and set(planted) <= set(eid.tolist())
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_sq8_codes(sq, codes)
    got, (scans,) = launches(ctx, ["sq8_scan"], lambda: idx.search_sq8(q[None], k))
    assert scans >= 1
    same(got, 0, eid, esc)


# dim 64: full = 4, one ring round — the ring is refilled from the next tile at once (the carried `tp` is never read: a lost
# `tp = tpn` shows from two rounds up — 768 here, 192 below); 768: the benchmark's row, 12 rounds;
# 80: full = 5, no ring — the plain row loop, dealt; 100: a tail group
@pytest.mark.parametrize("dim,metric", [(64, 0), (768, 0), (80, 0), (100, 0), (64, 2), (100, 2)])
def test_sq8_one_query_second_trip(vg, ctx, cus, dim, metric):
    """sq8_scan_kernel<DOT, 4>, two trips for the busiest waves: `tp = tpn` and the ring carried from tile to tile"""
    run_sq8_dealt(vg, ctx, cus, dim, metric, sh.SQ8_WAVES, 10)


@pytest.mark.parametrize("dim,metric,k,tie_run", [(64, 0, 10, 0), (192, 0, 10, 0), (192, 2, 10, 0), (64, 0, 130, 70)])
def test_sq8_one_query_eight_waves(vg, ctx, cus, dim, metric, k, tie_run):
    """sq8_scan_kernel<DOT, 8> with wg_rank_merge<8>, two trips; k = 130: three pages, 70 equal scores from both trips across
    the first page's end"""
    run_sq8_dealt(vg, ctx, cus, dim, metric, sh.SQ8_WIDE_WAVES, k, tie_run)


# ---- RaBitQ ---------------------------------------------------------------------------------------------------------------------
def rabitq_codes(rng, n, dim):
    """random sign bits, norms in [25, 30)"""
    cb = o.rabitq_code_bytes(dim)
    codes = rng.integers(0, 256, (n, cb), dtype=np.uint8)
    codes[:, cb - 4:] = (rng.random(n, dtype=np.float32) * 5 + 25).view(np.uint8).reshape(n, 4)
    return codes


def rabitq_query(rng, dim):
    return (rng.standard_normal(dim) * (27.0 / np.sqrt(dim))).astype(np.float32)     # |q| near the rows' norms


def rabitq_near(q, dim):
    nb = o.rabitq_code_bytes(dim) - 4
    signs = np.zeros(nb * 8, np.uint8)
    signs[:dim] = q >= 0

    def near(level):                                        # `level` sign bits flipped, spread over the row's words; norm 27
        b = signs.copy()
        b[spread(level, dim)] ^= 1
        return np.concatenate([np.packbits(b, bitorder="little"), np.array([27.0], np.float32).view(np.uint8)])
    return near


def run_rabitq_dealt(vg, ctx, cus, dim, want_trips, k, tie_run=0):
    n = sh.rows_for(want_trips, cus, 4, sh.RABITQ_WAVES)
    slices = sh.slices_for(n, cus, 4)
    plan, run = dealt_plan(n, slices, sh.RABITQ_WAVES, want_trips, tie_run)
    rng = np.random.default_rng(7000 + dim + k)
    codes = rabitq_codes(rng, n, dim)
    q = rabitq_query(rng, dim)
    planted = plant(codes, rabitq_near(q, dim), plan, run)
    eid, esc = o.flat_search_rabitq(codes, dim, q, k)
    assert eid.size == k and set(planted) <= set(eid.tolist())
    idx = vg.Index(ctx, n, dim)
    idx.set_rabitq_codes(codes)
    got, (one, mq) = launches(ctx, ["rabitq_scan", "rabitq_scan_mq"], lambda: idx.search_rabitq(q[None], k))
    assert one >= 1 and mq == 0
    same(got, 0, eid, esc)


@pytest.mark.parametrize("k,tie_run", [(10, 0), (130, 70)])
def test_rabitq_one_query_ring_three_trips(vg, ctx, cus, k, tie_run):
    """rabitq_scan_kernel, groups == 6: the ring of kRqTiles slots refilled kRqTiles steps ahead, three trips (slot 0 twice);
    k = 130: the floor key of the later pages inside the ring loop, 70 equal scores from all three trips across a page's end"""
    run_rabitq_dealt(vg, ctx, cus, 768, 3, k, tie_run)


# dim 128: one 16-byte group; 200: two; 1000: 128 bytes of sign bits, 8 groups
@pytest.mark.parametrize("dim,k,tie_run", [(128, 10, 0), (200, 10, 0), (1000, 10, 0), (200, 70, 60)])
def test_rabitq_one_query_generic_second_trip(vg, ctx, cus, dim, k, tie_run):
    """rabitq_scan_kernel's loop for groups != 6, dealt, two trips"""
    run_rabitq_dealt(vg, ctx, cus, dim, 2, k, tie_run)


@pytest.mark.parametrize("nq", [1, 3])
def test_rabitq_at_the_dimension_limit(vg, ctx, nq):
    """dim 8192: 64 groups, all of qbits[64] (one query) and of the batch kernel's query image"""
    n, dim, k = 300, 8192, 10
    rng = np.random.default_rng(8192 + nq)
    codes = rabitq_codes(rng, n, dim)
    q = np.stack([rabitq_query(rng, dim) for _ in range(nq)])
    codes[n - 1] = rabitq_near(q[0], dim)(2)
    idx = vg.Index(ctx, n, dim)
    idx.set_rabitq_codes(codes)
    got = idx.search_rabitq(q, k)
    for i in range(nq):
        eid, esc = o.flat_search_rabitq(codes, dim, q[i], k)
        assert i or eid[0] == n - 1
        same(got, i, eid, esc)


# ---- PQ ADC ---------------------------------------------------------------------------------------------------------------------
def adc_near(opq, q):
    t = opq.build_table(q).reshape(opq.m, -1)
    order = np.argsort(t, axis=1, kind="stable")

    def near(level):                                        # the nearest centroid everywhere, the second nearest in `level` sub-spaces
        c = order[:, 0].copy()
        p = spread(level, opq.m)
        c[p] = order[p, 1]
        return c.astype(np.uint8)
    return near


@pytest.mark.parametrize("dim,m,k,exhaustive,scans", [
    (768, 96, 10, False, 1),     # <6, true, true>: two tiles ahead, addresses clamped to the last tile
    (768, 96, 200, False, 2),    # every wave's 64 best (<6, true, true>, raw lists), select and verify; the flagged re-scan's launch
    (768, 96, 200, True, 1),     # <6, false, true>: the LDS-buffer scan
    (128, 16, 10, False, 1),     # <-1, true, true>
])
def test_adc_one_query_three_trips(vg, ctx, cus, dim, m, k, exhaustive, scans):
    from tests.test_gpu_adc import _mk, _random_pq
    n = sh.rows_for(3, cus, 1, sh.ADC_WAVES, sh.ADC_WAVES)
    slices = sh.slices_for(n, cus, 1, sh.ADC_WAVES)
    plan, run = dealt_plan(n, slices, sh.ADC_WAVES, 3)
    rng = np.random.default_rng(100 * m + k)
    opq = _random_pq(rng, dim, m)
    q = rng.standard_normal((2, dim)).astype(np.float32)
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    planted = plant(codes, adc_near(opq, q[0]), plan, run)
    eid, esc = o.flat_search_pq(opq, codes, q[0], k)
    assert eid.size == k and set(planted) <= set(eid.tolist())
    pq, idx = _mk(vg, ctx, opq, codes, n)
    if exhaustive:
        hooks.set_hook("VG_ADC_BIGK_EXHAUSTIVE", 1)
    try:
        got, (count,) = launches(ctx, ["pq_adc_scan"], lambda: idx.search_pq_adc(q[:1], k))
    finally:
        hooks.set_hook("VG_ADC_BIGK_EXHAUSTIVE", 0)
    assert count == scans
    same(got, 0, eid, esc)
    if k == 10 and m == 16:                                 # the same query as a row of a batch (sliced, not dealt): the same answer
        both = idx.search_pq_adc(q, k)
        assert np.array_equal(both[0][0], got[0][0]) and np.array_equal(bits(both[1][0]), bits(got[1][0]))


# ---- several queries: many trips per slice ----------------------------------------------------------------------------------------
def slice_plan(n, slices, waves_tiles, block, nq):
    """A several-query scan over n rows in `slices` contiguous slices, waves_tiles tiles per workgroup trip: preconditions, then
    winners in the first and the last tile of one slice and in the segment's last row."""
    tiles = sh.n_tiles(n)
    assert tiles // slices > 2 * waves_tiles and tiles % slices and nq > block      # several trips, uneven slices, several blocks
    s = slices // 2 + 1
    t0, t1 = tiles * s // slices, tiles * (s + 1) // slices
    return [(t0 * 64 + 1, 1), ((t1 - 1) * 64 + 62, 1), (t0 * 64 + 64 + 9, 2), (n - 1, 0)]


def checked_queries(nq):
    return [0, nq - 1, nq - 3, 1, nq // 3, nq // 2, nq // 2 + 1]


@pytest.mark.parametrize("dim,k", [(768, 10), (200, 70)])
def test_rabitq_batch_many_trips_per_slice(vg, ctx, cus, dim, k):
    """rabitq_scan_mq_kernel<6> / <0>: 1030 queries in blocks of 16 (the last of 6) over 20 000 rows"""
    n, nq = 20_000, 1030
    assert nq % sh.RABITQ_MQ == 6
    slices = sh.slices_for(n, cus, 4, units=(nq + sh.RABITQ_MQ - 1) // sh.RABITQ_MQ)
    plan = slice_plan(n, slices, sh.RABITQ_WAVES * 2, sh.RABITQ_MQ, nq)
    rng = np.random.default_rng(20_000 + dim)
    codes = rabitq_codes(rng, n, dim)
    q = np.stack([rabitq_query(rng, dim) for _ in range(nq)])
    check = checked_queries(nq)
    for j, c in enumerate(check[1:]):                       # the checked queries: query 0 with j + 1 signs turned, another length
        q[c] = q[0] * (1.0 + 0.01 * (j + 1))
        q[c, spread(j + 1, dim)] *= -1.0
    planted = plant(codes, rabitq_near(q[0], dim), plan, [])
    idx = vg.Index(ctx, n, dim)
    idx.set_rabitq_codes(codes)
    got, (one, mq) = launches(ctx, ["rabitq_scan", "rabitq_scan_mq"], lambda: idx.search_rabitq(q, k))
    assert one == 0 and mq >= 1
    for c in check:
        eid, esc = o.flat_search_rabitq(codes, dim, q[c], k)
        assert set(planted) <= set(eid.tolist())
        same(got, c, eid, esc)
    c = check[2]                                            # a query of the ragged block, alone: the one-query kernel, the same answer
    alone, (one, mq) = launches(ctx, ["rabitq_scan", "rabitq_scan_mq"], lambda: idx.search_rabitq(q[c:c + 1], k))
    assert one >= 1 and mq == 0
    assert np.array_equal(alone[0][0], got[0][c]) and np.array_equal(bits(alone[1][0]), bits(got[1][c]))


def test_sq8_batch_many_trips_per_slice(vg, ctx, cus):
    """sq8_scan_mq_kernel: 600 queries in groups of 4 over 20 000 rows of 100 dimensions (a tail group)"""
    n, dim, nq, k = 20_000, 100, 600, 10
    slices = sh.slices_for(n, cus, 4, units=(nq + sh.SQ8_MQ - 1) // sh.SQ8_MQ)
    plan = slice_plan(n, slices, sh.SQ8_WAVES, sh.SQ8_MQ, nq)
    rng = np.random.default_rng(600)
    sq, ref = sq8_quantizer(vg, ctx, rng, dim)
    q0, cq = sq8_query(rng, ref, dim, 0)
    codes = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    planted = plant(codes, sq8_near(cq), plan, [])
    q = (rng.standard_normal((nq, dim)) * 3).astype(np.float32)
    check = checked_queries(nq)
    for c in check:                                         # the checked queries: next to query 0, a hundredth of a code step off
        q[c] = q0 + (rng.standard_normal(dim) * 0.01 * ref.inv_scales).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_sq8_codes(sq, codes)
    got = idx.search_sq8(q, k)
    for c in check:
        eid, esc = o.flat_search_sq8(ref, codes, q[c], k)
        assert set(planted) <= set(eid.tolist())
        same(got, c, eid, esc)
    c = check[1]                                            # the last query alone: the one-query kernel, the same answer
    alone = idx.search_sq8(q[c:c + 1], k)
    assert np.array_equal(alone[0][0], got[0][c]) and np.array_equal(bits(alone[1][0]), bits(got[1][c]))
