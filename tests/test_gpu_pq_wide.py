"""PQ flat searches over a table that one LDS image does not hold (m > 96: dim / 8 sub-quantizers from 776 dimensions up) —
the probed, filtered and threshold scans walk the table in 96 KiB chunks (adc_wide_walk, vg_adc_wide.hpp) and answer what
they answer for a narrow table: the oracle's ids and score bits.  Sub-vector dimension 1 or 2 keeps the rows small; the
sizes sit at the chunk seams (6 groups per chunk, the m % 16 tail staged with the last chunk), at the batch seam (32 tiles
per workgroup step) and at partition bounds inside a tile.  Test hook VG_ADC_WIDE_ALWAYS sends narrow tables through the
same kernels, so wide and narrow answers meet on one index."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import flat_writer_ref as fref
from tests import hooks
from tests.probed_threshold_ref import L2, DOT, expected, rank_threshold

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
PQ = 1   # VG_SCAN_PQ
# 8 partitions over 6000 rows: one of 2500 rows (40 tiles: two batches of 32), one of 37 rows inside a single tile (it starts
# and ends mid-tile, fewer rows than one batch), an empty one, no inner offset at a multiple of 64
OFFSETS = np.array([0, 2500, 2537, 2537, 3300, 3391, 4700, 5130, 6000], np.uint32)
N = int(OFFSETS[-1])


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
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def random_pq(rng, dim, m):
    """random int8 codebooks, as tests/test_gpu_adc.py's"""
    opq = o.ProductQuantizer(dim, m, 256)
    cb = rng.integers(-128, 128, m * 256 * (dim // m)).astype(np.int8)
    scales = (rng.random(m) * 0.02 + 0.005).astype(np.float32)
    offsets = ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32)
    opq.set_codebooks(cb, scales, offsets)
    return opq


def make_segment(m, metric=L2, n=N, offsets=OFFSETS, sd=1, seed=0):
    """an oracle FlatSegment of n rows with random codes (a few rows repeated, so equal scores meet, also across a partition
    bound) and — offsets given — partitions at those offsets around random centroids"""
    rng = np.random.default_rng(1000 * m + 10 * metric + seed)
    dim = m * sd
    x = rng.standard_normal((n, dim)).astype(np.float32)
    codes = rng.integers(0, 256, (n, m)).astype(np.uint8)
    if n > 120:
        codes[100:110] = codes[100]
    if n > 2510:
        codes[2495:2505] = codes[2495]
    cent = None if offsets is None else (rng.standard_normal((len(offsets) - 1, dim)) * 0.7).astype(np.float32)
    return o.FlatSegment(x, dim, metric=metric, pq=random_pq(rng, dim, m), codes=codes, centroids=cent, part_offsets=offsets)


def gpu_index(vg, ctx, seg):
    idx = vg.Index(ctx, seg.n, seg.dim, vg.Metric(seg.metric))
    idx.set_vectors(seg.base)
    pq = vg.ProductQuantizer(ctx, seg.dim, seg.pq.m, 256)
    pq.set_codebooks(seg.pq.codebooks, seg.pq.scales, seg.pq.offsets)
    idx.set_pq_codes(pq, seg.codes)
    idx.quantizer = pq
    if seg.num_partitions:
        idx.set_partitions(seg.centroids, seg.part_offsets)
    return idx


def row_mask(mask, i):
    return None if mask is None else (mask if mask.ndim == 1 else mask[i])


def check_topk(res, seg, q, k, nprobes=0, mask=None, what=(), rows=None):
    ids, sc = res
    for i in (range(q.shape[0]) if rows is None else rows):
        eid, esc = seg.search(q[i], k, nprobes, row_mask(mask, i))
        r = eid.size
        assert np.array_equal(ids[i, :r], eid), (what, i, ids[i, :8], eid[:8])
        assert same_scores(sc[i, :r], esc), (what, i)
        assert np.all(ids[i, r:] == INVALID), (what, i)


def equal_results(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


# ---- filtered and probed scans --------------------------------------------------------------------------------------------
# m = 144: the first size the plain probe kernel cannot hold; 192: two full chunks; 200: 12 groups + a tail of 8; 208: 13 groups, a
# third chunk of one group
@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("m", [192, 200, 208, 144])
def test_probed_and_filtered(vg, ctx, m, metric):
    seg = make_segment(m, metric)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(m + metric)
    nq = 5
    q = rng.standard_normal((nq, seg.dim)).astype(np.float32)
    parts = seg.num_partitions
    assert parts == 8
    unmasked = {}
    for nprobes in (1, 3, parts):
        for k in (10, 64, 65, 130):   # 65, 130: pages of 64 results behind the previous page's last key
            res = idx.search_flat_probed(q, k, nprobes, PQ)
            check_topk(res, seg, q, k, nprobes, what=("probed", nprobes, k))
            unmasked[nprobes, k] = res
    for keep in (0.5, 0.03):
        for per_query in (False, True):
            mask = rng.random((nq, N) if per_query else N) < keep
            for nprobes, k in ((3, 10), (parts, 130), (1, 65), (parts, 64)):
                res = idx.search_flat_filtered(q, k, mask, nprobes, PQ)
                check_topk(res, seg, q, k, nprobes, mask, what=("filtered", keep, per_query, nprobes, k))
    for nprobes, k in ((3, 10), (parts, 130)):
        assert equal_results(idx.search_flat_filtered(q, k, np.ones(N, bool), nprobes, PQ), unmasked[nprobes, k])
        ids, sc = idx.search_flat_filtered(q, k, np.zeros((nq, N), bool), nprobes, PQ)
        assert np.all(ids == INVALID)


@pytest.mark.parametrize("m", [192, 200])
def test_many_queries_share_a_workgroup_between_ranges(vg, ctx, m):
    """100 queries: a workgroup takes a share of several probed ranges of its query, one after the other"""
    seg = make_segment(m)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(m)
    q = rng.standard_normal((100, seg.dim)).astype(np.float32)
    mask = rng.random((100, N)) < 0.3
    check_topk(idx.search_flat_probed(q, 10, 8, PQ), seg, q, 10, 8, what="probed", rows=range(0, 100, 9))
    check_topk(idx.search_flat_filtered(q, 70, mask, 5, PQ), seg, q, 70, 5, mask, what="filtered", rows=range(0, 100, 9))


@pytest.mark.parametrize("metric", [L2, DOT])
@pytest.mark.parametrize("m,n", [(192, 9000), (200, 9000), (144, 130), (208, 130)])
def test_unpartitioned_under_a_filter(vg, ctx, m, n, metric):
    """no partitions: the one range in pieces of at least 4096 rows (9000: two pieces, neither bound at a multiple of 64)"""
    seg = make_segment(m, metric, n=n, offsets=None)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(n + m)
    q = rng.standard_normal((4, seg.dim)).astype(np.float32)
    for keep in (0.5, 0.03):
        for mask in (rng.random(n) < keep, rng.random((4, n)) < keep):
            for k in (10, 64, 65, 130):
                check_topk(idx.search_flat_filtered(q, k, mask, 0, PQ), seg, q, k, 0, mask, what=(keep, mask.ndim, k))
    check_topk(idx.search_flat_filtered(q, 10, np.ones(n, bool), 0, PQ), seg, q, 10, what="all ones")
    assert np.all(idx.search_flat_filtered(q, 10, np.zeros(n, bool), 0, PQ)[0] == INVALID)


def test_few_rows_in_partitions(vg, ctx):
    """n = 130: three partitions inside three tiles"""
    off = np.array([0, 50, 50, 130], np.uint32)
    seg = make_segment(192, n=130, offsets=off)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(130)
    q = rng.standard_normal((3, seg.dim)).astype(np.float32)
    mask = rng.random((3, 130)) < 0.5
    for nprobes in (1, 3):
        for k in (10, 130):
            check_topk(idx.search_flat_probed(q, k, nprobes, PQ), seg, q, k, nprobes, what=(nprobes, k))
            check_topk(idx.search_flat_filtered(q, k, mask, nprobes, PQ), seg, q, k, nprobes, mask, what=(nprobes, k, "mask"))


# ---- threshold searches ---------------------------------------------------------------------------------------------------
def thresholds(seg, q, ranks, max_results, nprobes, mask, rerank):
    return np.array([rank_threshold(seg, q[i], ranks[i % len(ranks)], max_results, nprobes, row_mask(mask, i), rerank)
                     for i in range(q.shape[0])], np.float32)


def check_threshold(res, seg, q, thr, max_results, nprobes, mask, rerank, what=(), rows=None):
    ids, sc, cnt = res
    for i in (range(q.shape[0]) if rows is None else rows):
        eid, esc, kept = expected(seg, q[i], thr[i], max_results, nprobes, row_mask(mask, i), rerank)
        assert cnt[i] == kept, (what, i, int(cnt[i]), kept)
        assert np.array_equal(ids[i], eid), (what, i, ids[i][:8], eid[:8])
        assert same_scores(sc[i], esc), (what, i)


def run_threshold(idx, seg, q, ranks, max_results, nprobes=0, mask=None, rerank=False, what=()):
    thr = thresholds(seg, q, ranks, max_results, nprobes, mask, rerank)
    res = idx.search_flat_probed_threshold(q, thr, max_results, nprobes, PQ, rerank, mask)
    check_threshold(res, seg, q, thr, max_results, nprobes, mask, rerank, what)
    return thr, res


# m = 97: one chunk + a tail of 1; 112: 7 groups; rerank: the histogram and bin passes, then the exact re-score
@pytest.mark.parametrize("rerank", [False, True])
@pytest.mark.parametrize("m", [112, 97, 192, 200])
def test_threshold(vg, ctx, m, rerank):
    rng = np.random.default_rng(m + rerank)
    probed = make_segment(m)
    whole = o.FlatSegment(probed.base, probed.dim, pq=probed.pq, codes=probed.codes)
    q = rng.standard_normal((6, probed.dim)).astype(np.float32)
    shared, per_query = rng.random(N) < 0.4, rng.random((6, N)) < 0.05
    for seg, probes in ((whole, (0,)), (probed, (2, 8))):
        idx = gpu_index(vg, ctx, seg)
        for nprobes in probes:
            for max_results, mid in ((1, 1), (100, 40), (16384, 700)):   # 16384: more than the rows a query can see
                for mask in (None, shared, per_query):
                    thr, res = run_threshold(idx, seg, q, ["all", mid, "none"], max_results, nprobes, mask, rerank,
                                             what=(nprobes, max_results, None if mask is None else mask.ndim))
                    if m == 192 and not rerank and mask is None:
                        hooks.set_hook("VG_PTHR_FORCE_HIST", 1)
                        try:
                            forced = idx.search_flat_probed_threshold(q, thr, max_results, nprobes, PQ, False)
                        finally:
                            hooks.set_hook("VG_PTHR_FORCE_HIST", 0)
                        assert equal_results(forced, res), (nprobes, max_results)


@pytest.mark.parametrize("rerank", [False, True])
def test_threshold_many_queries_walk_several_batches(vg, ctx, rerank):
    """130 queries over the whole segment, 40 over every partition: few slices per range, so a workgroup walks more than one
    batch of 32 tiles"""
    probed = make_segment(192)
    whole = o.FlatSegment(probed.base, probed.dim, pq=probed.pq, codes=probed.codes)
    rng = np.random.default_rng(7 + rerank)
    for seg, nq, nprobes in ((whole, 130, 0), (probed, 40, 8)):
        idx = gpu_index(vg, ctx, seg)
        q = rng.standard_normal((nq, seg.dim)).astype(np.float32)
        mask = rng.random((nq, N)) < 0.3
        rows = range(0, nq, 13)
        thr = np.full(nq, np.inf, np.float32)
        for i in rows:
            thr[i] = rank_threshold(seg, q[i], 60, 100, nprobes, mask[i], rerank)
        res = idx.search_flat_probed_threshold(q, thr, 100, nprobes, PQ, rerank, mask)
        check_threshold(res, seg, q, thr, 100, nprobes, mask, rerank, what=(nq, nprobes), rows=rows)


# ---- narrow tables through the wide kernels -----------------------------------------------------------------------------------
# m = 8: the tail rows only; 16: one group; 96: exactly one chunk; 17: a group and a tail of 1
@pytest.mark.parametrize("m", [8, 16, 96, 17])
def test_hook_sends_narrow_tables_through_the_wide_kernels(vg, ctx, m):
    probed = make_segment(m, sd=2)
    whole = o.FlatSegment(probed.base, probed.dim, pq=probed.pq, codes=probed.codes)
    rng = np.random.default_rng(m)
    q = rng.standard_normal((5, probed.dim)).astype(np.float32)
    mask = rng.random((5, N)) < 0.2
    pidx, widx = gpu_index(vg, ctx, probed), gpu_index(vg, ctx, whole)
    thr = {(s, r): thresholds(seg, q, ["all", 30, "none"], 100, np_, mask, r)
           for s, seg, np_ in (("p", probed, 3), ("w", whole, 0)) for r in (False, True)}

    def everything():
        out = {}
        for k in (10, 130):
            out["probed", k] = pidx.search_flat_probed(q, k, 3, PQ)
            out["filtered", k] = pidx.search_flat_filtered(q, k, mask, 8, PQ)
            out["whole", k] = widx.search_flat_filtered(q, k, mask, 0, PQ)
        for r in (False, True):
            out["thr", "p", r] = pidx.search_flat_probed_threshold(q, thr["p", r], 100, 3, PQ, r, mask)
            out["thr", "w", r] = widx.search_flat_probed_threshold(q, thr["w", r], 100, 0, PQ, r, mask)
        return out
    narrow = everything()
    hooks.set_hook("VG_ADC_WIDE_ALWAYS", 1)
    try:
        wide = everything()
    finally:
        hooks.set_hook("VG_ADC_WIDE_ALWAYS", 0)
    for key in narrow:
        assert equal_results(narrow[key], wide[key]), key
    for k in (10, 130):
        check_topk(wide["probed", k], probed, q, k, 3, what=("probed", k))
        check_topk(wide["filtered", k], probed, q, k, 8, mask, what=("filtered", k))
        check_topk(wide["whole", k], whole, q, k, 0, mask, what=("whole", k))
    for r in (False, True):
        check_threshold(wide["thr", "p", r], probed, q, thr["p", r], 100, 3, mask, r, what=("thr p", r))
        check_threshold(wide["thr", "w", r], whole, q, thr["w", r], 100, 0, mask, r, what=("thr w", r))


# ---- NaN / Inf ---------------------------------------------------------------------------------------------------------------
def test_non_finite_queries_are_replayed(vg, ctx):
    """a NaN and an Inf query value: the table sums are NaN / Inf, the reference's heap decides — the replay stays wired behind
    the wide kernels"""
    seg = make_segment(192)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(3)
    q = rng.standard_normal((4, seg.dim)).astype(np.float32)
    q[1, 5] = np.nan
    q[2, 77] = np.inf
    mask = rng.random((4, N)) < 0.5
    for nprobes in (3, 8):
        check_topk(idx.search_flat_filtered(q, 10, mask, nprobes, PQ), seg, q, 10, nprobes, mask, what=("filtered", nprobes))
        thr = np.array([np.inf, np.inf, np.inf, rank_threshold(seg, q[3], 4, 50, nprobes, mask[3])], np.float32)
        res = idx.search_flat_probed_threshold(q, thr, 50, nprobes, PQ, False, mask)
        check_threshold(res, seg, q, thr, 50, nprobes, mask, False, what=("threshold", nprobes))


# ---- end to end: build, write, reopen ------------------------------------------------------------------------------------------
def test_built_segment_is_searchable(vg, ctx):
    """3000 x 1152 rows -> vg_flat_build with 6 partitions and PQ at the writer's default m = dim / 8 = 144 -> the image ->
    vg.Segment: search, search_filtered and search_threshold against the oracle over the codebooks and codes read back"""
    rng = np.random.default_rng(1152)
    n, dim, m, parts = 3000, 1152, 144, 6
    base = rng.standard_normal((n, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(base)
    gq = vg.ProductQuantizer(ctx, dim, m, 256)
    perm, _ = idx.flat_build(parts, gq, seed=5)
    img = idx.write_flat_segment(3)
    h = fref.parse_header(img)
    assert h["num_partitions"] == parts
    off = np.frombuffer(img, "<u4", parts + 1, h["part_off_off"])
    cent = np.frombuffer(img, "<f4", parts * dim, h["centroid_off"]).reshape(parts, dim)
    codes = np.frombuffer(img, np.uint8, n * m, h["codes_off"]).reshape(n, m)
    cb, sc, of = gq.codebooks()
    opq = o.ProductQuantizer(dim, m, 256)
    opq.set_codebooks(cb, sc, of)
    ref = o.FlatSegment(base[perm], dim, pq=opq, codes=codes, centroids=cent, part_offsets=off)
    seg = vg.Segment(ctx, img, "flat", verify_checksum=True)
    q = rng.standard_normal((4, dim)).astype(np.float32)
    mask = rng.random((4, n)) < 0.3
    for nprobes in (2, parts):
        check_topk(seg.search(q, 10, nprobes), ref, q, 10, nprobes, what=("search", nprobes))
        check_topk(seg.search_filtered(q, 70, mask, nprobes), ref, q, 70, nprobes, mask, what=("filtered", nprobes))
        for rerank in (False, True):
            thr = thresholds(ref, q, ["all", 20, "none"], 100, nprobes, mask, rerank)
            res = seg.search_threshold(q, thr, 100, nprobes=nprobes, rerank=rerank, mask=mask)
            check_threshold(res, ref, q, thr, 100, nprobes, mask, rerank, what=("threshold", nprobes, rerank))
    seg.close()


# ---- device buffers --------------------------------------------------------------------------------------------------------------
def test_device_buffers_on_a_callers_stream(vg, ctx):
    torch = pytest.importorskip("torch")
    seg = make_segment(192)
    idx = gpu_index(vg, ctx, seg)
    rng = np.random.default_rng(9)
    q = rng.standard_normal((5, seg.dim)).astype(np.float32)
    mask = rng.random((5, N)) < 0.4
    host = idx.search_flat_filtered(q, 70, mask, 3, PQ)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dq = torch.from_numpy(q).cuda()
        dm = torch.from_numpy(np.packbits(mask, axis=-1, bitorder="little")).cuda()
        out = (torch.zeros((5, 70), dtype=torch.int32, device="cuda"), torch.zeros((5, 70), dtype=torch.float32, device="cuda"))
        idx.search_flat_filtered(dq, 70, dm, 3, PQ, out=out, stream=side)
    side.synchronize()
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), host[0]) and np.array_equal(bits(out[1].cpu().numpy()), bits(host[1]))
    check_topk(host, seg, q, 70, 3, mask, what="host")
