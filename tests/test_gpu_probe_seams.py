"""The probed fp32 search (k_probe.hip) at the seams of its grouped paths, on the cases of tests/probe_cases.py: every batch is
answered three ways — the grouped matrix-core nomination (where the batch's shape takes it), the grouped scan (VG_PROBE_NO_GEMM)
and the pair-by-pair scan (VG_PROBE_NO_GROUP) — which must agree in ids and score bits on EVERY query, and a named handful of
queries (those steered at the seam partitions, the batch's first and last) must equal flat.Segment.Search of the oracle.  The
profile scope flat_probe_gemm tells that the path under test ran, and that the hooks kept it from running."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests import probe_cases as pc

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
SCOPE = "flat_probe_gemm"


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def three_ways(idx, q, k, nprobes, mask=None, gemm=True):
    """the same call with no hook, under VG_PROBE_NO_GEMM and under VG_PROBE_NO_GROUP: bit-identical on every query; `gemm`: the
    batch's shape takes the grouped nomination when nothing forbids it.  Returns the (ids, scores) of the run with no hook."""
    ctx = idx.ctx

    def run(hook):
        if hook:
            hooks.set_hook(hook, "1")
        ctx.profile_enable(True)
        try:
            ctx.profile_read(SCOPE)
            if mask is None:
                r = idx.search_flat_probed(q, k, nprobes, scan=idx.SCAN_F32)
            else:
                r = idx.search_flat_filtered(q, k, mask, nprobes, scan=idx.SCAN_F32)
            return r, ctx.profile_read(SCOPE)[0]
        finally:
            ctx.profile_enable(False)
            if hook:
                hooks.set_hook(hook, 0)

    (ids, sc), launches = run(None)
    assert (launches >= 1) if gemm else (launches == 0), launches
    for hook in ("VG_PROBE_NO_GEMM", "VG_PROBE_NO_GROUP"):
        (hid, hsc), launches = run(hook)
        assert launches == 0, (hook, launches)
        same = np.all(ids == hid, axis=1) & np.all(bits(sc) == bits(hsc), axis=1)
        assert same.all(), (hook, np.flatnonzero(~same)[:10].tolist())
    return ids, sc


def check_named(case, ids, sc, k, mask=None):
    """the named queries against the oracle: its rows in its order with its score bits, VG_INVALID_ID behind them"""
    seg = o.FlatSegment(case.x, case.cent.shape[1], metric=case.metric, centroids=case.cent, part_offsets=case.off)
    for i in case.named:
        eid, esc = seg.search(case.q[i], k, case.nprobes, mask=None if mask is None else mask[i])
        r = eid.size
        assert np.array_equal(ids[i, :r], eid), (case.name, i, k, ids[i, :12], eid[:12])
        assert np.array_equal(bits(sc[i, :r]), bits(esc)), (case.name, i, k)
        assert np.all(ids[i, r:] == INVALID), (case.name, i, k)


def index_of(vg, ctx, case):
    idx = vg.Index(ctx, case.x.shape[0], case.x.shape[1], vg.Metric(case.metric))
    idx.set_vectors(case.x)
    idx.set_partitions(case.cent, case.off)
    return idx


def ordered(ids, sc, metric):
    """every query's list is ordered by (score, row id) — largest scores first for Dot — with its valid rows in front"""
    valid = ids != INVALID
    assert np.all(valid[:, :-1] | ~valid[:, 1:])
    key = np.where(valid, -sc if metric != 0 else sc, 0.0).astype(np.float64)       # (the invalid tail's scores are +-Inf)
    both = valid[:, :-1] & valid[:, 1:]
    step = np.diff(key, axis=1)
    assert np.all((step > 0) | ~both | ((step == 0) & (np.diff(ids.astype(np.int64), axis=1) > 0)))


# ---- the tile-kind seam: 511 / 512 / 513 / 129 / 128 / 1 pairs per partition ----------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("nprobes", [1, 2])
def test_small_and_large_query_tiles_in_one_launch(vg, ctx, metric, nprobes):
    """partitions of up to kProbeSmallMax = 512 pairs go to the 128-query DMA32 tiles, larger ones to the 128 x 128 tiles, each
    kind with its own first-block prefix sums: 511, 512 and 513 pairs side by side, a whole small tile (128), one pair more (129)
    and a single pair; with two probes every query also lands on the 513-pair partition (1794 pairs, 15 tiles)"""
    case = pc.tile_kind_case(metric, nprobes)
    idx = index_of(vg, ctx, case)
    ids, sc = three_ways(idx, case.q, 10, nprobes, gemm=case.gemm)
    check_named(case, ids, sc, 10)
    ordered(ids, sc, metric)


def test_a_filter_per_query_follows_the_bucketing_across_both_tile_kinds(vg, ctx):
    """each bucketed pair reads its own query's filter (mask_off, probe_gather_queries_kernel) in the small-tile launch and in
    the 128 x 128 launch alike: a 50 % filter per query over the tile-kind layout"""
    case = pc.tile_kind_case(0, 1)
    idx = index_of(vg, ctx, case)
    mask = np.random.default_rng(7).random((case.q.shape[0], case.x.shape[0])) < 0.5
    ids, sc = three_ways(idx, case.q, 10, 1, mask=mask, gemm=case.gemm)
    check_named(case, ids, sc, 10, mask)
    for i in case.named:
        assert mask[i, ids[i]].all()


# ---- skew: the whole batch on one partition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprobes", [1, 2])
def test_the_whole_batch_on_the_largest_partition(vg, ctx, nprobes):
    """1300 queries on one of 16 partitions (two with nprobes = 2): 11 query tiles on one group, nothing on the others — the
    launches' grids cover them only through the "(pairs / 128) * largest partition" term of the host's bounds"""
    case = pc.skew_case(nprobes)
    idx = index_of(vg, ctx, case)
    ids, sc = three_ways(idx, case.q, 10, nprobes, gemm=case.gemm)
    check_named(case, ids, sc, 10)
    ordered(ids, sc, 0)
    inside = np.zeros(ids.shape, bool)
    for p in np.flatnonzero(case.pair_counts):
        inside |= (ids >= case.off[p]) & (ids < case.off[p + 1])
    assert inside.all()                                     # every query's rows come from the probed partitions


# ---- partitions of 1, 127, 128, 129, 0, 1024, 1025, 1023, 0, 2 rows --------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
def test_partition_row_counts_at_the_tile_seams(vg, ctx, metric):
    """one row tile and one row past it, 8 row tiles (one sampled tile) and one row past them, empty partitions with and without
    pairs; k = 100 is more than the 1- and 2-row partitions hold and k = 128 more than the 127-row one: the lists end in
    VG_INVALID_ID and stay ordered"""
    case, target = pc.row_seam_case(metric)
    idx = index_of(vg, ctx, case)
    rows = np.diff(case.off.astype(np.int64))
    for k in (10, 100, 128):
        ids, sc = three_ways(idx, case.q, k, 1, gemm=case.gemm)
        check_named(case, ids, sc, k)
        ordered(ids, sc, metric)
        have = np.minimum(rows[target], k)
        assert np.array_equal((ids != INVALID).sum(axis=1), have)
        for p in np.flatnonzero((rows <= k) & (np.array(pc.ROW_SEAM_COUNTS) > 0)):   # the short partitions: every row of theirs
            i = int(np.flatnonzero(target == p)[-1])
            assert np.array_equal(np.sort(ids[i, :rows[p]]), np.arange(case.off[p], case.off[p + 1]))


# ---- more partitions than the bucketing kernels have threads ---------------------------------------------------------------------
@pytest.mark.parametrize("parts,nq,nprobes", [(1500, 2400, 8), (1025, 20, 4)])
def test_more_partitions_than_bucketing_threads(vg, ctx, parts, nq, nprobes):
    """probe_bucket_scan_kernel and probe_group_kernel hand a thread ceil(parts / 1024) = 2 partitions: 1500 partitions under
    19 200 pairs take the nomination (and the grouped scan under VG_PROBE_NO_GEMM), 1025 under 80 pairs the grouped scan alone"""
    case = pc.many_parts_case(parts, nq, nprobes)
    idx = index_of(vg, ctx, case)
    ids, sc = three_ways(idx, case.q, 10, nprobes, gemm=case.gemm)
    check_named(case, ids, sc, 10)
    ordered(ids, sc, 0)


# ---- the grouped scan near its grid bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["ones", "ones2", "full"])
def test_grouped_scan_group_counts_near_the_grid_bound(vg, ctx, variant):
    """37 groups under a bound of pairs / 8 + parts = 41 (29 groups of one pair beside 8 of one partition; with two probes 28
    beside 3 + 6), and 30 partitions of 8 or 9 pairs: full groups beside groups of one"""
    case = pc.group_bound_case(variant)
    idx = index_of(vg, ctx, case)
    ids, sc = three_ways(idx, case.q, 10, case.nprobes, gemm=False)
    check_named(case, ids, sc, 10)
    ordered(ids, sc, 0)
    if variant == "ones":
        mask = np.random.default_rng(8).random((case.q.shape[0], case.x.shape[0])) < 0.5
        ids, sc = three_ways(idx, case.q, 10, case.nprobes, mask=mask, gemm=False)
        check_named(case, ids, sc, 10, mask)


# ---- more candidates than a pair keeps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("duplicates", [False, True])
@pytest.mark.parametrize("k", [10, 100])
def test_a_pair_with_more_candidates_than_the_cap(vg, ctx, duplicates, k):
    """every near row of one query lies in row tiles its partition's sample skips, so more than kProbeGemmCap = 2048 rows fall
    below its threshold: the pair is flagged and the query answered by the exact kernel (k <= 64: in place, through qfail; k = 100:
    the subset search), its neighbours in the batch keep their lists — distinct near rows and 2688 copies of one (a tie across
    the k-th place), with and without the bfloat16 filter"""
    case, _ = pc.overflow_case(duplicates)
    idx = index_of(vg, ctx, case)
    ids, sc = three_ways(idx, case.q, k, 1, gemm=case.gemm)
    check_named(case, ids, sc, k)
    idx.enable_bf16_filter(True)
    fid, fsc = three_ways(idx, case.q, k, 1, gemm=case.gemm)
    assert np.array_equal(ids, fid) and np.array_equal(bits(sc), bits(fsc))
    at = pc.OVERFLOW_AT
    lo, hi = int(case.off[1]), int(case.off[2])
    assert np.all((ids[at] >= lo) & (ids[at] < hi)) and np.all(((ids[at].astype(np.int64) - lo) // pc.GEMM_BN) % pc.SAMPLE_STRIDE != 0)
