"""Engine.SearchThreshold over flat segments with codes and IVF partitions on the GPU (vg_search_flat_probed_threshold,
vg_segment_search_threshold) vs the oracle's composition (tests/probed_threshold_ref.py): flat.Segment.Search(q, max_results,
nprobes, filter) with the segment's scan, Segment.Rerank, the engine's filter.  Every case compares ids, score bits, counts and
the padding; thresholds sit at oracle scores of chosen ranks, so boundaries are hit exactly."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks, segfile
from tests.probed_threshold_ref import L2, COS, DOT, candidates, expected, partitioned, pq_of, rank_threshold, sq8_of

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
F32, PQ, SQ8 = 0, 1, 2
NOT_READY = -9   # VG_ERR_NOT_READY


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same_scores(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def gpu_index(vg, ctx, seg, vectors=True):
    """the resident twin of an oracle FlatSegment: rows, the oracle's quantizer and codes, its partitions"""
    idx = vg.Index(ctx, seg.n, seg.dim, vg.Metric(seg.metric))
    if vectors:
        idx.set_vectors(seg.base)
    if seg.sq is not None:
        sq = vg.ScalarQuantizer(ctx, seg.dim)
        sq.set_bounds(seg.sq.mins, seg.sq.maxs)
        for mine, theirs in zip(sq.params(), (seg.sq.mins, seg.sq.maxs, seg.sq.scales, seg.sq.inv_scales)):
            assert same_scores(mine, theirs)
        idx.set_sq8_codes(sq, seg.codes)
        idx.quantizer = sq   # (outlives the index)
    if seg.pq is not None:
        pq = vg.ProductQuantizer(ctx, seg.dim, seg.pq.m, 256)
        pq.set_codebooks(seg.pq.codebooks, seg.pq.scales, seg.pq.offsets)
        idx.set_pq_codes(pq, seg.codes)
        idx.quantizer = pq
    if seg.num_partitions:
        idx.set_partitions(seg.centroids, seg.part_offsets)
    return idx


def scan_of(seg):
    return SQ8 if seg.sq is not None else PQ if seg.pq is not None else F32


def row_mask(mask, i):
    return None if mask is None else (mask if mask.ndim == 1 else mask[i])


def thresholds(seg, q, ranks, max_results, nprobes=0, mask=None, rerank=False):
    return np.array([rank_threshold(seg, q[i], ranks[i % len(ranks)], max_results, nprobes, row_mask(mask, i), rerank)
                     for i in range(q.shape[0])], np.float32)


def verify(res, seg, q, thr, max_results, nprobes=0, mask=None, rerank=False, what=()):
    ids, sc, cnt = res
    for i in range(q.shape[0]):
        eid, esc, kept = expected(seg, q[i], thr[i], max_results, nprobes, row_mask(mask, i), rerank)
        assert cnt[i] == kept, (what, i, int(cnt[i]), kept)
        assert np.array_equal(ids[i], eid), (what, i, ids[i][:12], eid[:12])
        assert same_scores(sc[i], esc), (what, i)


def run_and_verify(idx, seg, q, ranks, max_results, nprobes=0, mask=None, rerank=False, what=()):
    thr = thresholds(seg, q, ranks, max_results, nprobes, mask, rerank)
    res = idx.search_flat_probed_threshold(q, thr, max_results, nprobes, scan_of(seg), rerank, mask)
    verify(res, seg, q, thr, max_results, nprobes, mask, rerank, what)
    return thr, res


# ---- SQ8, unpartitioned -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("n,dim,max_results,mid", [
    (1000, 40, 100, 37),        # a 16-element group tail (40 % 16), a last tile of 1000 % 64 rows
    (20000, 32, 16384, 9000),   # "all": more than 16384 listed keys, the radix select
])
def test_sq8_whole_segment(vg, ctx, metric, n, dim, max_results, mid):
    rng = np.random.default_rng(n + dim + metric)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    sq, codes = sq8_of(x, dim)
    seg = o.FlatSegment(x, dim, metric=metric, sq=sq, codes=codes)
    idx = gpu_index(vg, ctx, seg)
    q9 = rng.standard_normal((9, dim)).astype(np.float32)   # one pass of 8 queries and one of 1
    for rerank in (False, True):
        run_and_verify(idx, seg, q9, ["all", "none", 1, mid], max_results, rerank=rerank, what=("nq9", rerank))
        run_and_verify(idx, seg, q9[:3], [mid, "all", 1], max_results, rerank=rerank, what=("nq3", rerank))


# ---- 7 partitions of unequal sizes, one of them empty, offsets at no multiple of 64 ----------------------------------------
class Probed:
    """the partitioned segments of this file, built once"""

    def __init__(self):
        self.segs = {}

    def rows(self, dim, metric):
        key = ("rows", dim, metric)
        if key not in self.segs:
            rng = np.random.default_rng(700 + dim + metric)
            self.segs[key] = partitioned(rng, 3000, dim, 7, metric, empty=(2,))
        return self.segs[key]

    def sq8(self, metric):
        key = ("sq8", metric)
        if key not in self.segs:
            x, cent, off = self.rows(64, metric)
            sq, codes = sq8_of(x, 64)
            self.segs[key] = o.FlatSegment(x, 64, metric=metric, sq=sq, codes=codes, centroids=cent, part_offsets=off)
        return self.segs[key]

    def f32(self, dim, metric):
        x, cent, off = self.rows(dim, metric)
        return o.FlatSegment(x, dim, metric=metric, centroids=cent, part_offsets=off)


@pytest.fixture(scope="module")
def probed():
    return Probed()


def test_the_partitioning_reaches_its_seams(probed):
    _, _, off = probed.rows(64, L2)
    sizes = np.diff(off.astype(np.int64))
    assert sizes[2] == 0 and np.count_nonzero(sizes) == 6 and len(set(sizes.tolist())) == 7
    assert all(int(v) % 64 != 0 for v in off[1:-1])


@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("nprobes", [1, 3, 7])
def test_sq8_probed(vg, ctx, probed, metric, nprobes):
    seg = probed.sq8(metric)
    idx = gpu_index(vg, ctx, seg)
    q = np.random.default_rng(nprobes).standard_normal((5, 64)).astype(np.float32)
    for max_results, mid in ((10, 5), (513, 200), (3000, 300)):
        for rerank in (False, True):
            run_and_verify(idx, seg, q, ["all", mid, 1, "none"], max_results, nprobes, rerank=rerank, what=(max_results, rerank))


@pytest.mark.parametrize("dim,metric", [(30, L2), (128, L2), (128, COS)])   # pairs from memory; rows in registers
def test_f32_probed(vg, ctx, probed, dim, metric):
    seg = probed.f32(dim, metric)
    idx = gpu_index(vg, ctx, seg)
    q = np.random.default_rng(dim).standard_normal((5, dim)).astype(np.float32)
    for nprobes in (1, 3, 7):
        for rerank in (False, True):   # 513: beyond vg_search_flat_probed's k
            run_and_verify(idx, seg, q, ["all", 200, 1, "none"], 513, nprobes, rerank=rerank, what=(nprobes, rerank))


# ---- PQ, L2 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [0, 5])
def test_pq(vg, ctx, parts):
    rng = np.random.default_rng(40 + parts)
    n, dim, m = 3000, 64, 8
    if parts:
        x, cent, off = partitioned(rng, n, dim, parts)
    else:
        x, cent, off = rng.standard_normal((n, dim)).astype(np.float32), None, None
    pq, codes = pq_of(x, dim, m)
    seg = o.FlatSegment(x, dim, pq=pq, codes=codes, centroids=cent, part_offsets=off)
    idx = gpu_index(vg, ctx, seg)
    q = rng.standard_normal((5, dim)).astype(np.float32)
    for nprobes in ((2, 5) if parts else (0,)):
        for rerank in (False, True):
            run_and_verify(idx, seg, q, ["all", 250, 1, "none"], 600, nprobes, rerank=rerank, what=(nprobes, rerank))


# ---- masks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("selectivity", [0.3, 0.02])
@pytest.mark.parametrize("shared", [False, True])
def test_masks(vg, ctx, probed, selectivity, shared):
    seg = probed.sq8(L2)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(int(selectivity * 100) + shared)
    q = rng.standard_normal((5, 64)).astype(np.float32)
    mask = rng.random(seg.n if shared else (5, seg.n)) < selectivity
    max_results, nprobes = 200, 2
    if selectivity < 0.1:   # fewer rows pass inside the probed partitions than max_results asks for
        assert candidates(seg, q[0], max_results, nprobes, row_mask(mask, 0))[0].size < max_results
    for rerank in (False, True):
        run_and_verify(idx, seg, q, ["all", 10, 1, "none"], max_results, nprobes, mask, rerank, what=(rerank,))
    fseg = probed.f32(128, L2)   # fp32 rows, the whole-range pieces of an unpartitioned segment under the same kind of filter
    whole = o.FlatSegment(fseg.base, 128)
    widx = gpu_index(vg, ctx, whole)
    wq = rng.standard_normal((9, 128)).astype(np.float32)
    wmask = rng.random(whole.n if shared else (9, whole.n)) < selectivity
    run_and_verify(widx, whole, wq, ["all", 20, 1, "none"], 100, 0, wmask, False)


# ---- ties at the cut -----------------------------------------------------------------------------------------------------
def tie_segments():
    rng = np.random.default_rng(66)
    x, cent, off = partitioned(rng, 1200, 16, 4, integer=True, dup=6)   # 200 distinct integer rows, six times each
    sq, codes = sq8_of(x, 16)
    yield "dup6", o.FlatSegment(x, 16, sq=sq, codes=codes, centroids=cent, part_offsets=off), 3
    yield "dup6-whole", o.FlatSegment(x, 16, sq=sq, codes=codes), 0
    same = np.tile(rng.standard_normal((1, 16)).astype(np.float32), (500, 1))   # one histogram bin holds everything
    sq, codes = sq8_of(same, 16)
    yield "identical", o.FlatSegment(same, 16, sq=sq, codes=codes), 0


@pytest.mark.parametrize("name,seg,nprobes", list(tie_segments()), ids=lambda v: v if isinstance(v, str) else None)
def test_ties_at_the_cut(vg, ctx, name, seg, nprobes):
    idx = gpu_index(vg, ctx, seg)
    q = np.rint(np.random.default_rng(5).standard_normal((4, 16)) * 1.5).astype(np.float32)
    max_results = 100
    cid, csc = candidates(seg, q[0], seg.n, nprobes)
    assert cid.size > max_results and csc[max_results - 1] == csc[max_results], "equal code scores straddle rank max_results"
    for rerank in (False, True):
        thr, plain = run_and_verify(idx, seg, q, ["all", 50, 98, "none"], max_results, nprobes, rerank=rerank, what=(name, rerank))
        hooks.set_hook("VG_PTHR_FORCE_HIST", 1)
        try:
            forced = idx.search_flat_probed_threshold(q, thr, max_results, nprobes, SQ8, rerank)
        finally:
            hooks.set_hook("VG_PTHR_FORCE_HIST", 0)
        verify(forced, seg, q, thr, max_results, nprobes, None, rerank, what=(name, rerank, "forced"))
        for a, b in zip(plain, forced):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), (name, rerank)


# ---- agreement with the existing entry points --------------------------------------------------------------------------------
def test_agrees_with_the_topk_scans(vg, ctx, probed):
    k = 300
    for seg in (probed.sq8(L2), probed.sq8(DOT), probed.f32(128, L2)):
        idx = gpu_index(vg, ctx, seg)
        q = np.random.default_rng(9).standard_normal((5, seg.dim)).astype(np.float32)
        t = np.float32(np.inf if seg.metric == L2 else -np.inf)
        mask = np.random.default_rng(10).random((5, seg.n)) < 0.5
        ids, sc, cnt = idx.search_flat_probed_threshold(q, t, k, 3, scan_of(seg))
        pid, psc = idx.search_flat_probed(q, k, 3, scan=scan_of(seg))
        assert np.array_equal(ids, pid) and np.array_equal(bits(sc), bits(psc)) and np.all(cnt == np.sum(pid != INVALID, axis=1))
        ids, sc, cnt = idx.search_flat_probed_threshold(q, t, k, 3, scan_of(seg), mask=mask)
        fid, fsc = idx.search_flat_filtered(q, k, mask, 3, scan=scan_of(seg))
        assert np.array_equal(ids, fid) and np.array_equal(bits(sc), bits(fsc)) and np.all(cnt == np.sum(fid != INVALID, axis=1))
    seg = probed.sq8(L2)
    whole = o.FlatSegment(seg.base, seg.dim, sq=seg.sq, codes=seg.codes)
    idx = gpu_index(vg, ctx, whole)
    q = np.random.default_rng(11).standard_normal((9, 64)).astype(np.float32)
    ids, sc, cnt = idx.search_flat_probed_threshold(q, np.inf, k, 0, SQ8)
    sid, ssc = idx.search_sq8(q, k)
    assert np.array_equal(ids, sid) and np.array_equal(bits(sc), bits(ssc)) and np.all(cnt == k)
    # an unpartitioned fp32 index: vg_search_flat_threshold's answer, thresholds included
    thr = thresholds(o.FlatSegment(seg.base, seg.dim), q, ["all", 100, 1, "none"], k)
    a = idx.search_flat_probed_threshold(q, thr, k, 0, F32)
    b = idx.search_flat_threshold(q, thr, k)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert 0 < a[2][1] < k


# ---- NaN / Inf -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_results", [10, 16384])
def test_non_finite_scores(vg, ctx, probed, max_results):
    rng = np.random.default_rng(max_results)
    # a NaN query value over the whole segment: every scan score is a NaN, the reference's heap decides (rerank: exact NaN too — left out)
    seg = probed.sq8(L2)
    whole = o.FlatSegment(seg.base, seg.dim, sq=seg.sq, codes=seg.codes)
    idx = gpu_index(vg, ctx, whole)
    q = rng.standard_normal((3, 64)).astype(np.float32)
    q[1, 5] = np.nan
    for scan_seg in (whole, o.FlatSegment(seg.base, seg.dim)):
        thr = np.array([np.inf, np.inf, rank_threshold(scan_seg, q[2], 4, max_results)], np.float32)
        res = idx.search_flat_probed_threshold(q, thr, max_results, 0, scan_of(scan_seg))
        verify(res, scan_seg, q, thr, max_results, what=("nan query", scan_of(scan_seg)))
    # an Inf SQ8 minimum: every code score is +Inf (ties the heap breaks), the exact scores are finite
    bad = o.ScalarQuantizer(64)
    mins, maxs = seg.sq.mins.copy(), seg.sq.maxs.copy()
    mins[7] = np.inf
    gsq = vg.ScalarQuantizer(ctx, 64)
    gsq.set_bounds(mins, maxs)
    for dst, src in zip((bad.mins, bad.maxs, bad.scales, bad.inv_scales), gsq.params()):
        dst[:] = src
    bad.trained = True
    bseg = o.FlatSegment(seg.base, 64, sq=bad, codes=seg.codes, centroids=seg.centroids, part_offsets=seg.part_offsets)
    bidx = vg.Index(ctx, bseg.n, 64)
    bidx.set_vectors(bseg.base)
    bidx.set_sq8_codes(gsq, bseg.codes)
    bidx.set_partitions(bseg.centroids, bseg.part_offsets)
    fq = rng.standard_normal((3, 64)).astype(np.float32)
    for rerank in (False, True):
        thr = thresholds(bseg, fq, ["all", 3, "none"], max_results, 3, None, rerank)
        res = bidx.search_flat_probed_threshold(fq, thr, max_results, 3, SQ8, rerank)
        verify(res, bseg, fq, thr, max_results, 3, None, rerank, what=("inf minimum", rerank))
    # an fp32 row holding Inf, inside the partition the first query probes first
    fseg = probed.f32(128, L2)
    x = fseg.base.copy()
    pq_ = rng.standard_normal((3, 128)).astype(np.float32)
    first = int(np.argmin(((fseg.centroids - pq_[0]) ** 2).sum(1)))
    x[int(fseg.part_offsets[first]) + 3, 9] = np.inf
    iseg = o.FlatSegment(x, 128, centroids=fseg.centroids, part_offsets=fseg.part_offsets)
    iidx = gpu_index(vg, ctx, iseg)
    thr = thresholds(iseg, pq_, ["all", 5, "all"], max_results, 2)
    res = iidx.search_flat_probed_threshold(pq_, thr, max_results, 2, F32)
    verify(res, iseg, pq_, thr, max_results, 2, what=("inf row",))


# ---- a caller's stream, device buffers at an odd element offset ---------------------------------------------------------------
def test_own_stream_and_offset_buffers(vg, ctx, probed):
    import torch
    from tests import devbuf
    seg = probed.sq8(L2)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(21)
    q = rng.standard_normal((5, 64)).astype(np.float32)
    mask = rng.random((5, seg.n)) < 0.4
    max_results, nprobes = 300, 3
    for rerank in (False, True):
        thr = thresholds(seg, q, ["all", 60, 1, "none"], max_results, nprobes, mask, rerank)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            dq, dt = devbuf.offset_like(q, 4), devbuf.offset_like(thr, 4)
            dm = devbuf.offset_like(np.packbits(mask, axis=-1, bitorder="little"), 1)
            out = (devbuf.offset_like(np.zeros((5, max_results), np.uint32), 4), devbuf.offset_like(np.zeros((5, max_results), np.float32), 4),
                   devbuf.offset_like(np.zeros(5, np.int32), 4))
            idx.search_flat_probed_threshold(dq, dt, max_results, nprobes, SQ8, rerank, mask=dm, out=out, stream=side)
        side.synchronize()
        res = (devbuf.to_host(out[0]).view(np.uint32), devbuf.to_host(out[1]), devbuf.to_host(out[2]))
        verify(res, seg, q, thr, max_results, nprobes, mask, rerank, what=("side stream", rerank))


# ---- limits --------------------------------------------------------------------------------------------------------------
def test_limits(vg, ctx):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((100, 8)).astype(np.float32)
    idx = vg.Index(ctx, 100, 8)
    idx.set_vectors(x)
    q = rng.standard_normal((2, 8)).astype(np.float32)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_flat_probed_threshold(q, 1.0, 16385)
    assert e.value.status == -5 and "16385" in e.value.message
    ids, sc, cnt = idx.search_flat_probed_threshold(q, np.inf, 16384)
    assert cnt.tolist() == [100, 100] and np.all(ids[:, 100:] == INVALID)
    with pytest.raises(vg.VecgoHipError) as e:   # no SQ8 codes
        idx.search_flat_probed_threshold(q, 1.0, 10, scan=SQ8)
    assert e.value.status == NOT_READY
    with pytest.raises(vg.VecgoHipError) as e:   # no PQ codes
        idx.search_flat_probed_threshold(q, 1.0, 10, scan=PQ)
    assert e.value.status == NOT_READY
    sq, codes = sq8_of(x, 8)
    bare = gpu_index(vg, ctx, o.FlatSegment(x, 8, sq=sq, codes=codes), vectors=False)
    bare.search_flat_probed_threshold(q, 1.0, 10, scan=SQ8)
    with pytest.raises(vg.VecgoHipError) as e:   # rerank without the fp32 rows
        bare.search_flat_probed_threshold(q, 1.0, 10, scan=SQ8, rerank=True)
    assert e.value.status == NOT_READY
    ham = vg.Index(ctx, 100, 8, vg.Metric.HAMMING)
    with pytest.raises(vg.VecgoHipError) as e:
        ham.search_flat_probed_threshold(q, 1.0, 10)
    assert e.value.status == -5
    # nq == 0 / max_results == 0 write nothing
    out = (np.full((2, 4), 7, np.uint32), np.full((2, 4), 7, np.float32), np.full(2, 7, np.int32))
    idx.search_flat_probed_threshold(q[:0], np.zeros(0, np.float32), 4, out=out)
    assert all(np.all(a == 7) for a in out)
    empty = (np.zeros((2, 0), np.uint32), np.zeros((2, 0), np.float32), np.full(2, 7, np.int32))
    idx.search_flat_probed_threshold(q, 1.0, 0, out=empty)
    assert np.all(empty[2] == 7)


# ---- the segment wrapper -------------------------------------------------------------------------------------------------
def test_segment_wrapper(vg, ctx, probed):
    ref = probed.sq8(L2)
    image = segfile.write_flat(ref.base, sq=(ref.sq.mins, ref.sq.maxs), codes=ref.codes, partitions=(ref.centroids, ref.part_offsets))
    seg = vg.Segment(ctx, image)
    assert seg.info.num_partitions == 7
    idx = gpu_index(vg, ctx, ref)
    q = np.random.default_rng(31).standard_normal((5, 64)).astype(np.float32)
    mask = np.random.default_rng(32).random(ref.n) < 0.5
    for rerank in (False, True):
        thr = thresholds(ref, q, ["all", 100, 1, "none"], 513, 3, mask, rerank)
        got = seg.search_threshold(q, thr, 513, nprobes=3, rerank=rerank, mask=mask)
        verify(got, ref, q, thr, 513, 3, mask, rerank, what=("segment", rerank))
        want = idx.search_flat_probed_threshold(q, thr, 513, 3, SQ8, rerank, mask)
        for a, b in zip(got, want):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    seg.close()
