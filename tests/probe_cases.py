"""Partitioned segments and query batches built to land on the seams of the probed fp32 search (k_probe.hip): exact row counts
per partition, exact (query, probe) pair counts per partition, and one partition whose near rows all sit in row tiles the
threshold sample skips.  Nothing here touches the GPU: every case is checked against the oracle's own probe selection
(tests/test_probe_cases_cpu.py) and then run by tests/test_gpu_probe_seams.py.

The constants restate the sources (test_probe_cases_cpu.py compares them):
  GEMM_BM x GEMM_BN     the 128-query x 128-row tile of the grouped GEMM (vg_flat_gemm.hpp)
  SAMPLE_STRIDE         every 8th row tile of a partition is sampled for the pairs' thresholds (k_probe.hip)
  SMALL_MAX             a partition with up to 512 pairs takes the SMALL_TILE_Q = kProbeRB * 32 = 128-query DMA32 tiles,
                        a larger one the 128 x 128 tiles (probe_bucket_scan_kernel)
  PROBE_QB              pairs per group of the grouped scan (vg_internal.hpp)
  GEMM_CAP              candidates kept per pair; a pair with more is flagged and its query re-scanned (k_flat.hip)
  GEMM_MAX_K            largest k of the grouped nomination (vg_internal.hpp)
  MIN_PAIRS_PER_PART    pairs >= 12 * parts sends a batch to the grouped nomination (ProbedGemmPath::plan)"""
import collections

import numpy as np

from oracle import oracle as o

GEMM_BM = 128
GEMM_BN = 128
SAMPLE_STRIDE = 8
SMALL_MAX = 512
SMALL_TILE_Q = 128
PROBE_QB = 8
GEMM_CAP = 2048
GEMM_MAX_K = 160
MIN_PAIRS_PER_PART = 12
MAX_PAIRS = 65535
GROUP_MIN_PAIRS = 16
BUCKET_THREADS = 1024       # the one-workgroup bucketing kernels: ceil(parts / 1024) partitions per thread

RADIUS = 4.0                # |centroid|
ROW_NOISE = 0.5             # a partition's rows around its centroid
QUERY_NOISE = 0.02          # a steered query around its centroid: far inside the nearest-centroid margin


def takes_gemm(pairs, parts, k=10):
    """ProbedGemmPath::plan's shape test for an fp32 batch with dim % 4 == 0"""
    return k <= GEMM_MAX_K and MIN_PAIRS_PER_PART * parts <= pairs <= MAX_PAIRS


def takes_group(pairs):
    """ProbedScanPath::plan's group_ok on a partitioned segment"""
    return pairs >= GROUP_MIN_PAIRS


def scan_groups(pair_counts):
    """groups of up to PROBE_QB pairs probe_group_kernel cuts, and the mq kernel's grid bound min(pairs, pairs / 8 + parts)"""
    pc = np.asarray(pair_counts, np.int64)
    pairs = int(pc.sum())
    return int(((pc + PROBE_QB - 1) // PROBE_QB).sum()), min(pairs, pairs // PROBE_QB + pc.size)


def gemm_blocks(pair_counts, rows_per_part):
    """what probe_bucket_scan_kernel sums ([sample, main] of the 128 x 128 tiles, then of the small tiles) beside the host's
    grid bounds for the same batch (ProbedGemmPath::plan): ((used), (bound))"""
    used, sums, maxs = [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]
    for cnt, rows in zip(pair_counts, rows_per_part):
        nt = -(-int(rows) // GEMM_BN)
        nst = -(-nt // SAMPLE_STRIDE)
        per = (-(-nst // 8) * 8, -(-nt // 8) * 8, nst, nt)
        for i in range(4):
            sums[i] += per[i]
            maxs[i] = max(maxs[i], per[i])
        if cnt and rows:
            if cnt <= SMALL_MAX:
                mt = -(-int(cnt) // SMALL_TILE_Q)
                used[2] += mt * nst
                used[3] += mt * nt
            else:
                mt = -(-int(cnt) // GEMM_BM)
                used[0] += mt * per[0]
                used[1] += mt * per[1]
    pairs = int(np.sum(pair_counts))
    bound = [sums[0] + pairs // GEMM_BM * maxs[0], sums[1] + pairs // GEMM_BM * maxs[1],
             sums[2] + pairs // SMALL_TILE_Q * maxs[2], sums[3] + pairs // SMALL_TILE_Q * maxs[3]]
    return tuple(used), tuple(bound)


# ---- centroids -----------------------------------------------------------------------------------------------------------------
def spread_centroids(rng, parts, dim):
    """random directions at one radius: for L2 and for Dot a point near centroid p has p as its closest, by a margin of
    RADIUS^2 (1 - cos) against QUERY_NOISE * RADIUS"""
    c = rng.standard_normal((parts, dim))
    c *= RADIUS / np.linalg.norm(c, axis=1, keepdims=True)
    return c.astype(np.float32)


def hub_centroids(parts, dim, hub):
    """Centroids whose SECOND closest is known too (parts <= dim): c_hub = R e_hub and c_p = R (e_p + a_p e_hub), a_p = 0.8 for
    the last partition that is not the hub and about 0.5 for the others.  For L2 (|c_p - c_hub|^2 = R^2 (1 + (1 - a_p)^2) against
    |c_p - c_j|^2 > 2 R^2) and for Dot (c_p.c_hub = a_p R^2 against c_p.c_j = a_p a_j R^2) alike, the order seen from c_p is p, hub,
    then the rest; seen from c_hub it is hub, then the last partition.  Every margin is above R^2 / 10, a steered query's noise
    moves a distance by about QUERY_NOISE * R."""
    assert parts <= dim and 0 <= hub < parts
    c = np.zeros((parts, dim))
    last = hub_second(parts, hub)[hub]
    for p in range(parts):
        c[p, p] = RADIUS
        if p != hub:
            c[p, hub] = RADIUS * (0.8 if p == last else 0.5 + 0.001 * p)
    return c.astype(np.float32)


def hub_second(parts, hub):
    """the second closest partition of a query steered at p, under hub_centroids"""
    last = parts - 1 if hub != parts - 1 else parts - 2
    return [last if p == hub else hub for p in range(parts)]


# ---- the builders --------------------------------------------------------------------------------------------------------------
def laid_out(rng, dim, rows_per_part, metric, cent=None):
    """(x, cent, off) with exactly rows_per_part[p] rows in partition p: its centroid plus noise.  The reference scans the
    ranges it is given (flat/segment.go:727-749) and never checks that a row lies in its nearest partition, so any layout
    with rising offsets is a legal segment."""
    rows_per_part = np.asarray(rows_per_part, np.int64)
    parts = rows_per_part.size
    if cent is None:
        cent = spread_centroids(rng, parts, dim)
    assert cent.shape == (parts, dim)
    off = np.concatenate(([0], np.cumsum(rows_per_part))).astype(np.uint32)
    x = np.repeat(cent, rows_per_part, axis=0) + (ROW_NOISE * rng.standard_normal((int(off[-1]), dim))).astype(np.float32)
    x = np.ascontiguousarray(x, np.float32)
    assert x.shape[0] == off[-1] and np.array_equal(np.diff(off.astype(np.int64)), rows_per_part)
    return x, cent, off


def probes_of(q, cent, nprobes, metric):
    """the oracle's FindClosestCentroids for every query: [nq, min(nprobes, parts)]"""
    dim = cent.shape[1]
    return np.stack([o.find_closest_centroids(q[i], cent, dim, nprobes, metric) for i in range(q.shape[0])]).astype(np.int64)


def steered_queries(rng, cent, counts, nprobes, metric, expect=None):
    """Queries of which exactly counts[p] have partition p as their closest, in shuffled order.  Returns (q, target, pair_counts):
    target[i] is the partition query i was steered at and pair_counts[p] the (query, probe) pairs partition p receives under the
    ORACLE's probe selection.  The first probes must equal `counts`; with nprobes == 1 that fixes pair_counts, with more probes
    the case states what its centroids make of the further ones in `expect` (hub_centroids) and that is asserted too."""
    counts = np.asarray(counts, np.int64)
    parts, dim = cent.shape
    assert counts.size == parts
    target = rng.permutation(np.repeat(np.arange(parts), counts))
    q = (cent[target] + QUERY_NOISE * rng.standard_normal((target.size, dim))).astype(np.float32)
    pr = probes_of(q, cent, nprobes, metric)
    assert np.array_equal(pr[:, 0], target), "a steered query's closest centroid is not its own"
    assert all(len(set(row)) == row.size for row in pr)
    pair_counts = np.bincount(pr.ravel(), minlength=parts)
    if nprobes == 1:
        expect = counts if expect is None else expect
    if expect is not None:
        assert np.array_equal(pair_counts, np.asarray(expect, np.int64)), (pair_counts.tolist(), list(expect))
    return q, target, pair_counts


def hidden_from_sample(rng, dim, duplicates, tiles=24, before=1000, after=700):
    """Three partitions; the middle one (tiles * 128 rows, starting at row `before`, no multiple of 128) hides its near rows from
    the threshold sample: its row tiles 0, 8, 16, ... — counted from the PARTITION's first row, as the grouped GEMM counts them —
    hold far rows only, every other tile holds rows near one query.  The sampled threshold of that query (the 8th best sampled
    score; a deeper one for k > 48 lies higher still) therefore passes every near row: more than GEMM_CAP candidates.
    (16 tiles would leave 14 x 128 = 1792 unsampled rows, fewer than GEMM_CAP: hence 24, of which 21 are unsampled.)
    duplicates: the near rows are copies of one row, a tie across any k-th place.  L2.  Returns (x, cent, off, near_query, below):
    `below` = the partition's rows scoring strictly under that threshold."""
    rows = tiles * GEMM_BN
    hidden = tiles - -(-tiles // SAMPLE_STRIDE)
    assert before % GEMM_BN != 0 and hidden * GEMM_BN >= GEMM_CAP + 200
    x, cent, off = laid_out(rng, dim, [before, rows, after], 0)
    tile_of = np.arange(rows) // GEMM_BN
    near = tile_of % SAMPLE_STRIDE != 0
    part = x[off[1]:off[2]]                                         # (a view: the rows are written in place)
    part[~near] = cent[1] + (ROW_NOISE * 2 * rng.standard_normal((int((~near).sum()), dim))).astype(np.float32)
    if duplicates:
        part[near] = cent[1] + (0.01 * rng.standard_normal(dim)).astype(np.float32)
    else:
        part[near] = cent[1] + (0.01 * rng.standard_normal((int(near.sum()), dim))).astype(np.float32)
        assert np.unique(part[near], axis=0).shape[0] == near.sum() >= GEMM_CAP + 200
    query = (cent[1] + 0.001 * rng.standard_normal(dim)).astype(np.float32)
    score = ((part.astype(np.float64) - query.astype(np.float64)) ** 2).sum(axis=1)
    sampled = np.sort(score[~near])
    assert sampled.size == (tiles - hidden) * GEMM_BN
    below = int((score < sampled[7]).sum())
    assert below > GEMM_CAP, below
    # the same count with tiles taken at multiples of 128 of the SEGMENT would see near rows in its sample: the layout is
    # only adversarial for a sample that starts at the partition
    seg_tile = (np.arange(rows) + int(off[1])) // GEMM_BN
    assert (score[seg_tile % SAMPLE_STRIDE == 0] < sampled[0]).any()
    return x, cent, off, query, below


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# x, cent, off: the segment; q: the batch; named: the queries compared with the oracle (the others only between the three
# paths); pair_counts: per partition, by the oracle's probe selection; gemm: the batch takes the grouped nomination when no hook
# is set
Case = collections.namedtuple("Case", "name x cent off metric q nprobes named pair_counts gemm")


def _named(target, parts_of_interest, nq, cap=14):
    """the first and the last query steered at each partition of interest, and the first and last of the batch"""
    picked = [0, nq - 1]
    for p in parts_of_interest:
        at = np.flatnonzero(target == p)
        if at.size:
            picked += [int(at[0]), int(at[-1])]
    return sorted(set(picked))[:cap]


def _case(name, x, cent, off, metric, q, nprobes, named, pair_counts, k_max=10):
    pairs, parts = q.shape[0] * min(nprobes, cent.shape[0]), cent.shape[0]
    assert int(np.sum(pair_counts)) == pairs
    return Case(name, x, cent, off, metric, q, nprobes, named, np.asarray(pair_counts, np.int64), takes_gemm(pairs, parts, k_max))


TILE_KIND_COUNTS = [SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, SMALL_TILE_Q + 1, SMALL_TILE_Q, 1]


def tile_kind_case(metric, nprobes):
    """6 partitions of 1500 rows with 511 / 512 / 513 / 129 / 128 / 1 queries steered at them: the small-tile kind up to 512
    pairs, the 128 x 128 kind from 513, whole and broken query tiles of both in one launch.  nprobes = 2: every query's second
    partition is the 513-pair one (1794 pairs), whose own queries go on to the last partition (514: a second large group)."""
    rng = np.random.default_rng(1000 + 10 * metric + nprobes)
    dim, parts, hub = 32, 6, 2
    cent = hub_centroids(parts, dim, hub)
    x, cent, off = laid_out(rng, dim, [1500] * parts, metric, cent)
    expect = np.array(TILE_KIND_COUNTS)
    if nprobes == 2:
        for p, s in enumerate(hub_second(parts, hub)):
            expect[s] += TILE_KIND_COUNTS[p]
        assert expect.tolist() == [511, 512, 1794, 129, 128, 514]
    q, target, pc = steered_queries(rng, cent, TILE_KIND_COUNTS, nprobes, metric, expect)
    used, _ = gemm_blocks(pc, np.diff(off.astype(np.int64)))
    assert all(u > 0 for u in used)          # both kinds have workgroups in both stages
    return _case(f"tile_kind-m{metric}-np{nprobes}", x, cent, off, metric, q, nprobes, _named(target, range(parts), q.shape[0]), pc)


SKEW_ROWS = [300, 700, 1100, 500, 900, 8300, 400, 1300, 600, 800, 1000, 350, 1700, 450, 650, 750]


def skew_case(nprobes):
    """16 partitions, 1300 queries all steered at the largest one: 11 query tiles of 128 on one group, 15 empty groups — the
    grids' "(pairs / 128) * max" term is all that covers tiles 2..11 (8300 rows: 65 row tiles, 9 of them sampled, so that the
    SAMPLE launch too needs more workgroups than one query tile per partition comes to).  nprobes = 2: the same onto two partitions (the largest
    and the hub, 1300 pairs each)."""
    rng = np.random.default_rng(1100 + nprobes)
    dim, parts, big, hub = 32, len(SKEW_ROWS), 5, 12
    assert SKEW_ROWS[big] == max(SKEW_ROWS)
    cent = hub_centroids(parts, dim, hub)
    x, cent, off = laid_out(rng, dim, SKEW_ROWS, 0, cent)
    counts = np.zeros(parts, np.int64)
    counts[big] = 1300
    expect = counts.copy()
    if nprobes == 2:
        expect[hub] = 1300
    q, target, pc = steered_queries(rng, cent, counts, nprobes, 0, expect)
    used, bound = gemm_blocks(pc, SKEW_ROWS)
    sums = gemm_blocks(np.zeros(parts, np.int64), SKEW_ROWS)[1]
    assert used[0] > sums[0] and used[1] > sums[1]        # past the sum over partitions: the skew term is what is tested
    assert all(u <= b for u, b in zip(used, bound))
    nq = q.shape[0]
    return _case(f"skew-np{nprobes}", x, cent, off, 0, q, nprobes, [0, 1, 127, 128, 129, nq // 2, 1279, 1280, nq - 2, nq - 1], pc)


ROW_SEAM_ROWS = [1, GEMM_BN - 1, GEMM_BN, GEMM_BN + 1, 0, SAMPLE_STRIDE * GEMM_BN, SAMPLE_STRIDE * GEMM_BN + 1,
                 SAMPLE_STRIDE * GEMM_BN - 1, 0, 2]
ROW_SEAM_COUNTS = [130, 600, 131, 140, 20, 700, 135, 130, 0, 133]


def row_seam_case(metric):
    """partitions of 1, 127, 128, 129, 0, 1024, 1025, 1023, 0 and 2 rows (one row tile and one past it; 8 tiles = one sampled
    tile and one past it), each non-empty one probed by at least 130 queries, two by more than 512: both tile kinds see the
    seams.  One empty partition is probed too (its queries' lists are empty), the other by nobody."""
    rng = np.random.default_rng(1200 + metric)
    dim, parts = 32, len(ROW_SEAM_ROWS)
    x, cent, off = laid_out(rng, dim, ROW_SEAM_ROWS, metric, hub_centroids(parts, dim, 0))
    q, target, pc = steered_queries(rng, cent, ROW_SEAM_COUNTS, 1, metric)
    assert all(c >= 130 for c, r in zip(ROW_SEAM_COUNTS, ROW_SEAM_ROWS) if r) and sum(c > SMALL_MAX for c in ROW_SEAM_COUNTS) == 2
    named = sorted({0, q.shape[0] - 1} | {int(np.flatnonzero(target == p)[0]) for p in range(parts) if ROW_SEAM_COUNTS[p]})
    return _case(f"row_seams-m{metric}", x, cent, off, metric, q, 1, named, pc, k_max=128), target


def many_parts_case(parts, nq, nprobes):
    """more partitions than the bucketing kernels have threads (two per thread): 8 rows each, every 7th empty"""
    rng = np.random.default_rng(1300 + parts)
    dim = 32
    rows = np.where(np.arange(parts) % 7 == 6, 0, 8)
    x, cent, off = laid_out(rng, dim, rows, 0)
    assert -(-parts // BUCKET_THREADS) == 2
    at = rng.choice(parts, size=nq, replace=nq > parts)
    at[:3] = (0, parts - 1, BUCKET_THREADS)                # the first and last partition, and one from the threads' second halves
    at[3] = 6                                              # an empty one
    counts = np.bincount(at, minlength=parts)
    q, target, pc = steered_queries(rng, cent, counts, nprobes, 0)
    named = _named(target, (0, parts - 1, BUCKET_THREADS, 6), nq, cap=10)
    return _case(f"parts{parts}", x, cent, off, 0, q, nprobes, named, pc)


def group_bound_case(variant):
    """30 partitions, batches of the grouped scan alone (fewer than 12 pairs per partition):
    "ones": 90 queries x 1 probe, 29 partitions with exactly 1 pair and one with 61 — 29 + 8 = 37 groups under a grid bound of
            min(90, 90 / 8 + 30) = 41, the most groups 90 pairs over 30 partitions can make;
    "ones2": 45 queries x 2 probes — a query's two probes differ, so no partition can hold more than 45 of the 90 pairs: 28
            partitions with 1 pair, one with 17, the hub with 45, again 28 + 3 + 6 = 37 groups;
    "full": every partition 8 or 9 pairs: a full group beside a group of one."""
    rng = np.random.default_rng({"ones": 1401, "ones2": 1402, "full": 1403}[variant])
    dim, parts, hub = 32, 30, 7
    cent = hub_centroids(parts, dim, hub)
    x, cent, off = laid_out(rng, dim, [200 + 37 * (p % 5) for p in range(parts)], 0, cent)
    if variant == "ones":
        counts = np.ones(parts, np.int64)
        counts[hub] = 61
        nprobes, expect, groups = 1, counts, 37
    elif variant == "ones2":
        counts = np.ones(parts, np.int64)
        counts[hub] = 16
        expect = np.ones(parts, np.int64)
        expect[hub], expect[parts - 1] = 45, 17
        nprobes, groups = 2, 37
    else:
        counts = np.array([8 + p % 2 for p in range(parts)], np.int64)
        nprobes, expect, groups = 1, counts, 45
    q, target, pc = steered_queries(rng, cent, counts, nprobes, 0, expect)
    ng, gmax = scan_groups(pc)
    assert ng == groups and ng <= gmax and (variant == "full" or gmax - ng == 4)
    assert takes_group(int(pc.sum())) and not takes_gemm(int(pc.sum()), parts)
    return _case(f"group_bound-{variant}", x, cent, off, 0, q, nprobes, _named(target, (hub, 0, parts - 1), q.shape[0]), pc)


OVERFLOW_NQ, OVERFLOW_AT = 200, 100


def overflow_case(duplicates):
    """hidden_from_sample with 200 queries: the near query at index 100 between ordinary ones steered at the two other partitions
    (a few more at the hidden partition's centroid region, far from the near rows' query)"""
    rng = np.random.default_rng(1500 + int(duplicates))
    x, cent, off, near_q, below = hidden_from_sample(rng, 32, duplicates)
    q, target, pc = steered_queries(rng, cent, [110, 0, OVERFLOW_NQ - 110], 1, 0)
    q[OVERFLOW_AT] = near_q
    pr = probes_of(q, cent, 1, 0)
    assert pr[OVERFLOW_AT, 0] == 1
    pc = np.bincount(pr.ravel(), minlength=3)
    assert pc[1] == 1
    named = [0, OVERFLOW_AT - 2, OVERFLOW_AT - 1, OVERFLOW_AT, OVERFLOW_AT + 1, OVERFLOW_AT + 2, OVERFLOW_NQ - 1]
    return _case(f"overflow-dup{int(duplicates)}", x, cent, off, 0, q, 1, named, pc, k_max=100), below
