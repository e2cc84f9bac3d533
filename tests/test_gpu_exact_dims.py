"""The exact fp32 scorers of vg_exact.hpp at the dimensions where their block loops split differently (tests/exact_dims.py: DIMS and
the loop model; tests/test_exact_dims_cpu.py holds DIMS against the classes): every form, through a caller of each, bit for bit
against the oracle.

  kBatch             squared_l2_batch / dot_batch                     exact_pair16<DOT, kBatch, STREAM>       plain form
  kBounded           squared_l2_bounded_batch                         exact_pair16<false, kBounded, STREAM> + exact_l2_bounded_partial16
  kPair from memory  score_candidates, rerank, normalize_l2           exact_pair16<DOT, kPair>                plain form
  one row in regs    search_flat, 1 and 3 queries (flat_scan_small)   exact_rowregs16<DOT>   where regs_form(dim), else (and under
                     VG_FLAT_NO_SCAN) the nomination + exact_pair16 re-score
  two rows in regs   search_hnsw_brute under a shared mask / VG_BRUTE_NO_FLAT (brute_dist_mq_kernel) and the grouped fp32 probe
                     (probe_scan_f32_mq_kernel)                       exact_rowregs16x2<DOT> where brute_mq(dim), else exact_pair16
  HNSW walk          ef 64: LDS heaps                                 exact_l2_both16<false, false> / exact_pair16<true, kPair>
                     ef 513 > kHnswLdsEf: split heaps, query in LDS   exact_l2_both16<false, true> / exact_pair16<DOT, kPair, false, true>
  Vamana walk        k 10                                             exact_pair16<DOT, kPair>

Rows and queries are standard normal, so no two scores tie and (score, id) order is the oracle's order."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import exact_dims as ed
from tests import hooks
from tests.test_gpu_brute import _check as brute_check
from tests.test_gpu_brute import _oidx as brute_oracle
from tests.test_gpu_hnsw_scorers import case as hnsw_case
from tests.test_gpu_hnsw_scorers import check as hnsw_check
from tests.test_gpu_probe import check as probe_check
from tests.test_gpu_probe import partitioned
from tests.test_gpu_vamana_large_k import check as vamana_check
from tests.test_gpu_vamana_scorers import case as vamana_case

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
N, NQ, K = 601, 5, 10                       # odd: the last pair of rows of the two-row form is a row and padding
QLDS_111 = [d for d in ed.DIMS if ed.trips(d, "qlds") == (1, 1, 1)][0]


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


_rows, _indexes = {}, {}


def rows(dim):
    """(base [N, dim], queries [NQ, dim]) of one dimension, drawn once and left unchanged"""
    if dim not in _rows:
        rng = np.random.default_rng(7000 + dim)
        _rows[dim] = (rng.standard_normal((N, dim)).astype(np.float32), rng.standard_normal((NQ, dim)).astype(np.float32))
    return _rows[dim]


def index(vg, ctx, dim, metric):
    key = (dim, metric)
    if key not in _indexes:
        idx = vg.Index(ctx, N, dim, vg.Metric(metric))
        idx.set_vectors(rows(dim)[0])
        _indexes[key] = idx
    return _indexes[key]


def best(scores, ids, metric, k):
    """the k best of (scores, ids) by (score, id): smallest first under L2, largest first under Cosine / Dot"""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.uint32)
    order = np.lexsort((ids, -scores if metric else scores))[:k]
    return ids[order], scores[order]


@pytest.mark.parametrize("dim", ed.DIMS)
def test_batch(vg, ctx, dim):
    base, q = rows(dim)
    for n in (1, 17, 33):
        t = base[40:40 + n].ravel()
        assert np.array_equal(bits(vg.squared_l2_batch(ctx, q[0], t, dim)), bits(o.l2_batch(q[0], t, dim))), n
        assert np.array_equal(bits(vg.dot_batch(ctx, q[0], t, dim)), bits(o.dot_batch(q[0], t, dim))), n


@pytest.mark.parametrize("dim", ed.DIMS)
def test_bounded(vg, ctx, dim):
    """value and flag; a squared distance of two standard-normal rows is 2 dim +- sqrt(8 dim): every pair exceeds 1.0 dim (and leaves
    the block loop early where there is more than one block), about half exceed 2.0 dim, none 3.0 dim"""
    base, q = rows(dim)
    n = 33
    t = base[100:100 + n]
    rng = np.random.default_rng(dim)
    full = [o.l2_bounded(q[1], t[i], np.inf)[0] for i in range(n)]
    over = partial = 0
    for bounds in (1.0 * dim, 2.0 * dim, 3.0 * dim, ((1.0 + 2.0 * rng.random(n)) * dim).astype(np.float32)):
        d, e = vg.squared_l2_bounded_batch(ctx, q[1], t.ravel(), dim, bounds)
        for i in range(n):
            want, exc = o.l2_bounded(q[1], t[i], float(np.float32(bounds if np.ndim(bounds) == 0 else bounds[i])))
            assert bits(d[i]) == bits(want) and bool(e[i]) == exc, (dim, i, d[i], want, e[i], exc)
            over += exc
            partial += exc and bits(want) != bits(full[i])
    assert 0 < over < 4 * n                                  # both outcomes
    if ed.loops(dim, "plain").blocks >= 2:
        assert partial > 0                                   # the early exit's partial sum was asked for


@pytest.mark.parametrize("metric", [0, 1, 2], ids=["l2", "cosine", "dot"])
@pytest.mark.parametrize("dim", ed.DIMS)
def test_pair_from_memory(vg, ctx, dim, metric):
    base, q = rows(dim)
    if metric == 1:                                          # Cosine: the dot product of rows normalised by the library
        got = base.copy()
        ok = vg.normalize_l2(ctx, got, dim)
        for i in range(0, N, 13):
            want, wok = o.normalize_l2(base[i])
            assert bool(ok[i]) == wok and np.array_equal(bits(got[i]), bits(want)), i
        base, q = got, np.stack([o.normalize_l2(v)[0] for v in q])
        idx = vg.Index(ctx, N, dim, vg.Metric(1))
        idx.set_vectors(base)
    else:
        idx = index(vg, ctx, dim, metric)
    rng = np.random.default_rng(dim + metric)
    nq, nc = 3, 40
    cand = np.stack([rng.permutation(N)[:nc] for _ in range(nq)]).astype(np.uint32)
    sc = idx.score_candidates(q[:nq], cand)
    ids, scores = idx.rerank(q[:nq], cand, K)
    for qi in range(nq):
        exp = o.rerank_f32(base, dim, q[qi], cand[qi], metric)
        assert np.array_equal(bits(sc[qi]), bits(exp)), qi
        eid, esc = best(exp, cand[qi], metric, K)
        assert np.array_equal(ids[qi], eid) and np.array_equal(bits(scores[qi]), bits(esc)), qi
    if metric == 1:
        idx.close()


@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
@pytest.mark.parametrize("dim", ed.DIMS)
def test_one_row_in_registers(vg, ctx, dim, metric):
    """search_flat with 1 and 3 queries: the small-batch scan where regs_form(dim), the from-memory kernels elsewhere and under
    VG_FLAT_NO_SCAN; the same answer, the oracle's, from both"""
    base, q = rows(dim)
    idx = index(vg, ctx, dim, metric)
    every = np.arange(N, dtype=np.uint32)
    want = [best(o.rerank_f32(base, dim, q[qi], every, metric), every, metric, K) for qi in range(3)]
    for no_scan in (0, 1):
        hooks.set_hook("VG_FLAT_NO_SCAN", no_scan)
        try:
            for nq in (1, 3):
                ids, sc = idx.search_flat(q[:nq], K)
                for qi in range(nq):
                    assert np.array_equal(ids[qi], want[qi][0]), (no_scan, nq, qi)
                    assert np.array_equal(bits(sc[qi]), bits(want[qi][1])), (no_scan, nq, qi)
        finally:
            hooks.set_hook("VG_FLAT_NO_SCAN", 0)


@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
@pytest.mark.parametrize("dim", ed.DIMS)
def test_two_rows_in_registers_brute(vg, ctx, dim, metric):
    """5 queries over 601 rows.  A mask shared by fewer than 8 queries takes the distance matrix of brute_dist_mq_kernel where
    brute_mq(dim) (the one-row kernel elsewhere); unmasked the flat search answers, and the matrix again under VG_BRUTE_NO_FLAT"""
    base, q = rows(dim)
    idx = index(vg, ctx, dim, metric)
    oidx = brute_oracle(base, metric)
    mask = np.random.default_rng(dim).random(N) < 0.5
    mask[N - 1] = True                                       # the row whose partner is padding takes part
    for mode in (0, 1):
        brute_check(idx, oidx, q, K, mode, mask)
        brute_check(idx, oidx, q, K, mode, None)
        hooks.set_hook("VG_BRUTE_NO_FLAT", 1)
        try:
            brute_check(idx, oidx, q, K, mode, None)
        finally:
            hooks.set_hook("VG_BRUTE_NO_FLAT", 0)


@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
@pytest.mark.parametrize("dim", ed.DIMS)
def test_two_rows_in_registers_probe(vg, ctx, dim, metric):
    """10 queries x 2 probes over 2 partitions: 20 pairs are enough to be grouped by partition (16) and too few for the matrix-core
    nomination (12 per partition): probe_scan_f32_mq_kernel where brute_mq(dim), one pass per pair elsewhere and under
    VG_PROBE_NO_GROUP.  A partition's 10 pairs make a full group of 8 and one of 2; its rows are cut into at most 32 slices, of
    which a 16-lane group scores rows i and i + 4 together: two partitions of some 350 rows leave slices of about 11, so the second
    row of the pair is a row (with six partitions of 100 it was padding nearly everywhere)"""
    rng = np.random.default_rng(300 + dim + metric)
    n, parts, nprobes = 700, 2, 2
    x, cent, off = partitioned(rng, n, dim, parts, metric)
    q = rng.standard_normal((10, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(x)
    idx.set_partitions(cent, off)
    seg = o.FlatSegment(x, dim, metric=metric, centroids=cent, part_offsets=off)
    for no_group in (0, 1):
        hooks.set_hook("VG_PROBE_NO_GROUP", no_group)
        try:
            ids, sc = idx.search_flat_probed(q, K, nprobes, scan=idx.SCAN_F32)
        finally:
            hooks.set_hook("VG_PROBE_NO_GROUP", 0)
        probe_check(ids, sc, seg, q, K, nprobes)
    idx.close()


# ---- the walks: tests/test_gpu_hnsw_scorers.py's and tests/test_gpu_vamana_scorers.py's cases at these dimensions (their graphs come
# from the first 32 coordinates, so the set-up costs the same at any dimension) ---------------------------------------------------------
KEF = [(10, 64), (10, 513)]                 # LDS heaps: the plain form; split heaps (ef > kHnswLdsEf): the QLDS form
assert KEF[0][1] <= ed.HNSW_LDS_EF < KEF[1][1]


@pytest.mark.parametrize("k,ef", KEF)
@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
@pytest.mark.parametrize("dim", ed.DIMS)
def test_hnsw_walk(vg, ctx, dim, metric, k, ef):
    idx, oidx, search, q, dead = hnsw_case(vg, ctx, "f32", dim, metric)
    hnsw_check(search, oidx, q, k, ef)


@pytest.mark.parametrize("k,ef", KEF)
@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
def test_hnsw_walk_strict_pass_inf_query(vg, ctx, metric, k, ef):
    """the STRICT instance is another instantiation of the same scorers: an Inf in one coordinate of one query"""
    idx, oidx, search, q, dead = hnsw_case(vg, ctx, "f32", QLDS_111, metric)
    q = q.copy()
    q[2, QLDS_111 // 3] = np.inf
    assert oidx.search(q[2], k, ef)[2].pops >= 1
    hnsw_check(search, oidx, q, k, ef)


@pytest.mark.parametrize("k,ef", KEF)
@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
def test_hnsw_walk_strict_pass_tombstones(vg, ctx, metric, k, ef):
    idx, oidx, search, q, dead = hnsw_case(vg, ctx, "f32", QLDS_111, metric)
    oidx.set_tombstones(dead)
    idx.set_hnsw_tombstones(dead)
    try:
        ids = hnsw_check(search, oidx, q, k, ef)[0]
        assert not dead[ids[ids != INVALID]].any()
    finally:                                                 # (the case is cached)
        oidx.set_tombstones(None)
        idx.set_hnsw_tombstones(None)


@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
@pytest.mark.parametrize("dim", ed.DIMS)
def test_vamana_walk(vg, ctx, dim, metric):
    idx, ov, q, masks, metric = vamana_case(vg, ctx, "f32", dim, metric)
    vamana_check(idx, ov, q, K, 0, metric=metric)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask30"])
@pytest.mark.parametrize("metric", [0, 2], ids=["l2", "dot"])
def test_vamana_walk_strict_pass_inf_query(vg, ctx, metric, masked):
    """the Vamana walk has a filter where the HNSW walk has tombstones: an Inf query with and without one"""
    idx, ov, q, masks, metric = vamana_case(vg, ctx, "f32", QLDS_111, metric)
    q = q.copy()
    q[2, QLDS_111 // 3] = np.inf
    assert ov.search(q[2], K)[2].pops >= 1
    vamana_check(idx, ov, q, K, 0, mask=masks if masked else None, metric=metric)
