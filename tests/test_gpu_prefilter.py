"""vg_mask_to_rows and vg_search_flat_prefilter (the engine's bitmap strategy, engine/search.go:602-736) on the device.
Every check is exact: row lists against np.flatnonzero, ids and score bits against the oracle's flat segment under the same
filter (finite data: the heap policy cannot matter) and against tests/prefilter_ref.py where a score is a NaN.  The oracle is
asked once per (query, mask) for the deepest k; a smaller k is a prefix of that answer (scores are totally ordered)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as o
from tests import devbuf
from tests import prefilter_ref as ref

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
UNSUPPORTED, INVALID_ARG = -5, -1


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def same_scores(a, b):
    """score bits, except that a NaN's sign and payload are the instruction set's, not the algorithm's (the header's "NaN scores")"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def pack(m):
    return np.packbits(np.asarray(m, np.bool_), axis=-1, bitorder="little")


def status_of(vg, fn):
    with pytest.raises(vg.VecgoHipError) as e:
        fn()
    return e.value.status, e.value.message


# ---- vg_mask_to_rows ---------------------------------------------------------------------------------------------------
def _row_seams():
    import vecgo_amd
    t = vecgo_amd.MASK_ROWS_TILE_ROWS
    return sorted({1, 7, 8, 9, 63, 64, 65, t - 1, t, t + 1, 2 * t + 5})


MASK_KINDS = ("none", "all", "first", "last", "half", "sparse")


def mask_of(kind, rows, rng):
    m = np.zeros(rows, np.bool_)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "half":
        m = rng.random(rows) < 0.5
    elif kind == "sparse":
        m = rng.random(rows) < 0.01
    return m


def junk_tail(packed, rows):
    """set the bits at or above `rows` in each mask's last byte: they are not rows"""
    if rows % 8:
        packed[..., -1] |= np.uint8((0xFF << (rows % 8)) & 0xFF)
    return packed


def check_rows(vg, ctx, masks_bool, packed_arg, rows, what):
    """every out_stride seam for one batch of masks, as handed over in packed_arg (numpy or torch, any layout)"""
    nq = masks_bool.shape[0]
    want = [np.flatnonzero(m).astype(np.uint32) for m in masks_bool]
    cmax = max(w.size for w in want)
    for out_stride in sorted({max(cmax - 1, 0), cmax, cmax + 3}):
        ids, cnt = vg.mask_to_rows(ctx, packed_arg, rows, out_stride=out_stride)
        ids, cnt = devbuf.to_host(ids).view(np.uint32).reshape(nq, out_stride), devbuf.to_host(cnt)
        assert cnt.tolist() == [w.size for w in want], (what, out_stride)          # the full count, truncated or not
        for q in range(nq):
            kept = min(want[q].size, out_stride)
            assert np.array_equal(ids[q, :kept], want[q][:kept]), (what, out_stride, q)
            assert (ids[q, kept:] == INV).all(), (what, out_stride, q)


@pytest.mark.parametrize("rows", _row_seams())
def test_mask_to_rows_seams(vg, ctx, rows):
    import torch
    rng = np.random.default_rng(rows)
    nbytes = (rows + 7) // 8
    for kind in MASK_KINDS:                                     # one mask, every kind, device and host
        m = mask_of(kind, rows, rng)[None, :]
        p = junk_tail(pack(m), rows)
        check_rows(vg, ctx, m, torch.from_numpy(p).cuda(), rows, (kind, "device"))
        check_rows(vg, ctx, m, p, rows, (kind, "host"))
        check_rows(vg, ctx, m, p[0], rows, (kind, "host, 1-D"))
    m = np.stack([mask_of(MASK_KINDS[(q + 1) % 6], rows, rng) for q in range(5)])   # five masks, ragged counts
    p = junk_tail(pack(m), rows)
    check_rows(vg, ctx, m, torch.from_numpy(p).cuda(), rows, "5 device")
    check_rows(vg, ctx, m, p, rows, "5 host")
    # an odd byte address and an odd stride: byte loads, the same lists
    stride = nbytes + 3 + (nbytes % 2)
    assert stride % 2 == 1
    flat = np.full(1 + 5 * stride, 0xFF, np.uint8)
    view = flat[1:].reshape(5, stride)[:, :nbytes]
    view[:] = p
    assert view.ctypes.data % 2 == 1 and view.strides[0] == stride
    check_rows(vg, ctx, m, view, rows, "5 host, odd")
    dflat = torch.from_numpy(flat).cuda()
    dview = dflat[1:].view(5, stride)[:, :nbytes]
    assert dview.data_ptr() % 2 == 1 and dview.stride(0) == stride
    check_rows(vg, ctx, m, dview, rows, "5 device, odd")
    # count only; no query
    _, cnt = vg.mask_to_rows(ctx, torch.from_numpy(p).cuda(), rows, out_stride=0)
    assert cnt.cpu().tolist() == m.sum(axis=1).tolist()
    lib = ctx._lib
    assert lib.vg_mask_to_rows(ctx._h, None, C.c_int64(0), C.c_int64(0), C.c_int64(rows), None, C.c_int64(4), None, None) == 0


def test_mask_to_rows_without_rows(vg, ctx):
    out = np.zeros((2, 3), np.uint32)
    cnt = np.full(2, 7, np.int64)
    st = ctx._lib.vg_mask_to_rows(ctx._h, None, C.c_int64(0), C.c_int64(2), C.c_int64(0), C.c_void_p(out.ctypes.data), C.c_int64(3),
                                  C.c_void_p(cnt.ctypes.data), None)
    assert st == 0 and cnt.tolist() == [0, 0] and (out == INV).all()


# ---- vg_search_flat_prefilter against the oracle -------------------------------------------------------------------------
K_DEEP = 600


class Case:
    """one index with its oracle twin and, per (query, mask), the oracle's answer at the deepest k"""

    def __init__(self, vg, ctx, x, dim, metric):
        self.x, self.dim, self.metric = np.ascontiguousarray(x, np.float32), dim, metric
        self.n = self.x.shape[0]
        self.idx = vg.Index(ctx, self.n, dim, vg.Metric(metric))
        self.idx.set_vectors(self.x)
        self.seg = o.FlatSegment(self.x, dim, metric=metric)
        self.memo = {}

    def want(self, key, q, mask, k_deep=K_DEEP):
        if key not in self.memo:
            self.memo[key] = self.seg.search(q, k_deep, 0, mask=mask)
        return self.memo[key]

    def check(self, q, k, masks, key, k_deep=K_DEEP, **kw):
        """masks: bool [n] (one for the batch) or [nq, n]; key names (queries, masks) for the memo"""
        ids, sc = self.idx.search_flat_prefilter(q, k, masks, **kw)
        ids, sc = devbuf.to_host(ids).view(np.uint32), devbuf.to_host(sc)
        assert ids.shape == (q.shape[0], k)
        for i in range(q.shape[0]):
            m = masks if masks.ndim == 1 else masks[i]
            wi, ws = self.want((key, i), q[i], m, k_deep)
            r = min(k, wi.size)
            assert np.array_equal(ids[i, :r], wi[:r]), (key, k, i)
            assert np.array_equal(bits(sc[i, :r]), bits(ws[:r])), (key, k, i)
            assert (ids[i, r:] == INV).all() and (sc[i, r:] == (np.inf if self.metric == o.METRIC_L2 else -np.inf)).all(), (key, k, i)
        return ids, sc


SHAPES = [(3000, 64, o.METRIC_L2), (2000, 100, o.METRIC_DOT), (900, 24, o.METRIC_COSINE), (1500, 25, o.METRIC_L2),
          (70000, 16, o.METRIC_L2)]
KS = (1, 10, 64, 65, 130, 512, 513)


@pytest.mark.parametrize("n,dim,metric", SHAPES)
def test_prefilter_equals_the_flat_segment(vg, ctx, n, dim, metric):
    rng = np.random.default_rng(n + dim)
    c = Case(vg, ctx, rng.standard_normal((n, dim)), dim, metric)
    q = rng.standard_normal((90, dim)).astype(np.float32)
    for keep in (0.5, 0.03):
        per_query = rng.random((90, n)) < keep
        for name, masks in (("shared", per_query[0]), ("each", per_query)):
            sub = (lambda cnt: masks if masks.ndim == 1 else masks[:cnt])
            key = (keep, name)
            ids, sc = c.check(q, 10, masks, key)                           # 90 queries: several query groups / workgroups
            for k in KS:                                                    # 5 queries: every selection size; k beyond the hits pads
                c.check(q[:5], k, sub(5), key)
            c.check(q[:1], 10, sub(1), key)
            c.check(q[:1], 65, sub(1), key)
            if n * keep > 16384:                                            # a list beyond the LDS sort: the radix select
                c.check(q[:5], K_DEEP, sub(5), key)
            # the same filter through the scan: bit for bit
            fid, fsc = c.idx.search_flat_filtered(q, 10, masks, 0, scan=c.idx.SCAN_F32)
            assert np.array_equal(ids, fid) and np.array_equal(bits(sc), bits(fsc)), key
            fid, fsc = c.idx.search_flat_filtered(q[:5], 64, sub(5), 0, scan=c.idx.SCAN_F32)
            pid, psc = c.idx.search_flat_prefilter(q[:5], 64, sub(5))
            assert np.array_equal(pid, fid) and np.array_equal(bits(psc), bits(fsc)), key
    # packed masks where they lie on the device equal the host path
    import torch
    dm = torch.from_numpy(pack(per_query)).cuda()
    c.check(q, 10, per_query, (0.03, "each"))
    did, dsc = c.idx.search_flat_prefilter(torch.from_numpy(q).cuda(), 10, dm)
    hid, hsc = c.idx.search_flat_prefilter(q, 10, per_query)
    assert np.array_equal(devbuf.raw(did), devbuf.raw(hid)) and np.array_equal(devbuf.raw(dsc), devbuf.raw(hsc))


def exact_mask(rng, n, length):
    m = np.zeros(n, np.bool_)
    m[rng.choice(n, length, replace=False)] = True
    return m


def test_list_lengths_at_the_group_and_chunk_seams(vg, ctx):
    rng = np.random.default_rng(3)
    ch = vg.PREFILTER_CHUNK_ROWS
    lengths = [0, 1, 15, 16, 17, ch - 1, ch, ch + 1, 2 * ch + 1]
    n, dim = 2000, 64
    c = Case(vg, ctx, rng.standard_normal((n, dim)), dim, o.METRIC_L2)
    q = rng.standard_normal((len(lengths), dim)).astype(np.float32)
    ragged = np.stack([exact_mask(rng, n, ln) for ln in lengths])        # one batch, every length: a ragged CSR block
    for k in (10, 300):
        c.check(q, k, ragged, "ragged")
    for j, ln in enumerate(lengths):                                      # one list of that length for a batch of 5
        for k in (10, 300):
            c.check(q[:5], k, ragged[j], ("shared", ln))
        c.check(q[:1], 10, ragged[j], ("shared", ln))


@pytest.mark.parametrize("metric", [o.METRIC_L2, o.METRIC_DOT])
def test_eightfold_duplicated_rows_tie_by_row_id(vg, ctx, metric):
    rng = np.random.default_rng(8)
    n, dim = 2000, 32
    x = np.repeat(rng.standard_normal((n // 8, dim)).astype(np.float32), 8, axis=0)[rng.permutation(n)]
    c = Case(vg, ctx, x, dim, metric)
    q = rng.standard_normal((6, dim)).astype(np.float32)
    masks = rng.random((6, n)) < 0.5
    for k in (10, 65, 130):
        c.check(q, k, masks, "each")
        c.check(q, k, masks[0], "shared")


def test_k_16384_sorts_a_whole_list_in_lds(vg, ctx):
    rng = np.random.default_rng(16384)
    n, dim = 40000, 16
    c = Case(vg, ctx, rng.standard_normal((n, dim)), dim, o.METRIC_L2)
    q = rng.standard_normal((2, dim)).astype(np.float32)
    masks = rng.random((2, n)) < 0.5
    assert 16384 < masks.sum(axis=1).min()
    c.check(q, 16384, masks, "each", k_deep=16384)
    c.check(q, 16384, masks[0], "shared", k_deep=16384)


def test_partitions_are_ignored(vg, ctx):
    from tests.test_gpu_probe import partitioned
    rng = np.random.default_rng(77)
    n, dim = 3000, 64
    x, cent, off = partitioned(rng, n, dim, 7)
    c = Case(vg, ctx, x, dim, o.METRIC_L2)          # (the oracle twin has no partitions)
    c.idx.set_partitions(cent, off)
    q = rng.standard_normal((9, dim)).astype(np.float32)
    masks = rng.random((9, n)) < 0.1
    c.check(q, 10, masks, "each")
    c.check(q, 10, masks[0], "shared")


# ---- NaN scores: the engine's heap ----------------------------------------------------------------------------------------
def check_ref(idx, x, dim, metric, q, k, masks):
    ids, sc = idx.search_flat_prefilter(q, k, masks)
    for i in range(q.shape[0]):
        m = masks if masks.ndim == 1 else masks[i]
        wi, ws = ref.search(x, dim, metric, q[i], k, m)
        r = wi.size
        assert np.array_equal(ids[i, :r], wi), (k, i, ids[i, :r], wi)
        assert same_scores(sc[i, :r], ws), (k, i)
        assert (ids[i, r:] == INV).all()


@pytest.mark.parametrize("metric", [o.METRIC_L2, o.METRIC_DOT])
def test_nan_scores_follow_the_engine_heap(vg, ctx, metric):
    rng = np.random.default_rng(9 + metric)
    n, dim = 600, 40
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    masks = rng.random((3, n)) < 0.3
    listed, hidden = 5, 300
    masks[:, listed] = True
    masks[:, hidden] = False
    clean = vg.Index(ctx, n, dim, vg.Metric(metric))
    clean.set_vectors(x)
    before = [clean.search_flat_prefilter(q, k, masks) for k in (4, 70)]
    # a NaN in a row no mask lists: the row is never scored; the answers are the finite ones (through the replay)
    xh = x.copy()
    xh[hidden, 3] = np.nan
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(xh)
    for (bi, bs), k in zip(before, (4, 70)):
        ids, sc = idx.search_flat_prefilter(q, k, masks)
        assert np.array_equal(ids, bi) and np.array_equal(bits(sc), bits(bs)), k     # (no NaN among them)
        check_ref(idx, xh, dim, metric, q, k, masks)
    # a NaN in a listed row, early in the row order: it enters the heap while the heap fills
    xl = x.copy()
    xl[listed, 7] = np.nan
    idx.set_vectors(xl)
    for k in (4, 70):
        check_ref(idx, xl, dim, metric, q, k, masks)
        check_ref(idx, xl, dim, metric, q, k, masks[0])
    # a NaN in one query: every score of that query is a NaN, the others answer as before
    qn = q.copy()
    qn[1, 5] = np.nan
    for k in (4, 70):
        check_ref(clean, x, dim, metric, qn, k, masks)


def test_pop_then_push_decides_a_nan_case(vg, ctx):
    """the case of tests/test_prefilter_cpu.py: ReplaceTop would answer rows {3, 1, 2}, the engine's loop {3, 4, 1}"""
    from tests.test_prefilter_cpu import nan_case
    x, q, k = nan_case()
    idx = vg.Index(ctx, 5, 4, vg.Metric.L2)
    idx.set_vectors(x)
    m = np.ones(5, np.bool_)
    ids, sc = idx.search_flat_prefilter(q[None, :], k, m)
    wi, ws = ref.search(x, 4, o.METRIC_L2, q, k, m, "pop_push")
    ri, _ = ref.search(x, 4, o.METRIC_L2, q, k, m, "replace_top")
    assert np.array_equal(ids[0], wi) and same_scores(sc[0], ws)
    assert set(ids[0].tolist()) != set(ri.tolist())


# ---- trivial sizes and refusals ---------------------------------------------------------------------------------------------
def test_empty_masks_sizes_and_refusals(vg, ctx):
    rng = np.random.default_rng(1)
    n, dim = 500, 32
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((4, dim)).astype(np.float32)
    for metric, pad in ((vg.Metric.L2, np.inf), (vg.Metric.DOT, -np.inf)):
        idx = vg.Index(ctx, n, dim, metric)
        idx.set_vectors(x)
        for masks in (np.zeros(n, np.bool_), np.zeros((4, n), np.bool_)):
            ids, sc = idx.search_flat_prefilter(q, 7, masks)
            assert (ids == INV).all() and (sc == pad).all()
    # nq == 0 / k == 0: nothing is written
    ids, sc = np.full((4, 7), 123, np.uint32), np.full((4, 7), 4.5, np.float32)
    p = pack(np.ones(n, np.bool_))
    args = lambda nq, k: (idx._h, C.c_void_p(q.ctypes.data), C.c_int64(nq), C.c_int32(k), C.c_void_p(p.ctypes.data), C.c_int64(0),
                          C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), None)
    assert ctx._lib.vg_search_flat_prefilter(*args(0, 7)) == 0
    assert ctx._lib.vg_search_flat_prefilter(*args(4, 0)) == 0
    assert (ids == 123).all() and (sc == 4.5).all()
    # an index without rows: padding only
    empty = vg.Index(ctx, 0, dim, vg.Metric.L2)
    ids, sc = empty.search_flat_prefilter(q, 3, np.zeros(0, np.bool_))
    assert (ids == INV).all() and (sc == np.inf).all()
    # refusals
    st, msg = status_of(vg, lambda: idx.search_flat_prefilter(q, 16385, np.ones(n, np.bool_)))
    assert st == UNSUPPORTED and "16385" in msg
    ham = vg.Index(ctx, n, dim, vg.Metric.HAMMING)
    st, msg = status_of(vg, lambda: ham.search_flat_prefilter(q, 3, np.ones(n, np.bool_)))
    assert st == UNSUPPORTED and "Hamming" in msg
    assert ctx._lib.vg_search_flat_prefilter(idx._h, C.c_void_p(q.ctypes.data), C.c_int64(4), C.c_int32(7), None, C.c_int64(0),
                                             C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), None) == INVALID_ARG
    assert ctx._lib.vg_search_flat_prefilter(*args(4, 7)[:5], C.c_int64(3), *args(4, 7)[6:]) == INVALID_ARG     # a stride below a mask
    assert ctx._lib.vg_search_flat_prefilter(*args(-1, 7)) == INVALID_ARG
    bare = vg.Index(ctx, n, dim, vg.Metric.L2)
    st, _ = status_of(vg, lambda: bare.search_flat_prefilter(q, 3, np.ones(n, np.bool_)))
    assert st == -9, st   # VG_ERR_NOT_READY


# ---- device buffers: a caller's stream, views that are not 16-byte aligned ----------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_device_views_on_a_callers_stream(vg, ctx, shared):
    import torch
    rng = np.random.default_rng(4)
    n, dim, nq, k = 3000, 64, 12, 20
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    masks = rng.random(n if shared else (nq, n)) < 0.1
    idx = vg.Index(ctx, n, dim, vg.Metric.L2)
    idx.set_vectors(x)
    want_i, want_s = idx.search_flat_prefilter(q, k, masks)
    p = pack(masks)
    qv = devbuf.offset_like(q, 4)
    iv = devbuf.offset_like(np.zeros((nq, k), np.uint32), 4)
    sv = devbuf.offset_like(np.zeros((nq, k), np.float32), 4)
    md = devbuf.whole(np.zeros_like(p))
    q_real, m_real = devbuf.whole(q), devbuf.whole(p)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    devbuf.late_inputs(stream, [qv, md], [q_real, m_real])      # poison (NaN queries, every row listed) until the stream gets there
    idx.search_flat_prefilter(qv, k, md, out=(iv, sv), stream=stream)
    stream.synchronize()
    assert np.array_equal(devbuf.raw(iv), devbuf.raw(want_i)) and np.array_equal(devbuf.raw(sv), devbuf.raw(want_s))


def test_mask_to_rows_only_enqueues_with_device_buffers(vg, ctx):
    """the masks' producer is still running on the caller's stream when the call returns; the lists are right once it is done"""
    import torch
    rng = np.random.default_rng(12)
    rows = 2 * vg.MASK_ROWS_TILE_ROWS + 5
    m = rng.random((3, rows)) < 0.2
    p = pack(m)
    want = [np.flatnonzero(r) for r in m]
    width = max(w.size for w in want) + 2
    md, real = devbuf.whole(np.zeros_like(p)), devbuf.whole(p)
    out = torch.empty((3, width), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    vg.mask_to_rows(ctx, md, rows, out=out, stream=stream)       # (the first call on a stream may allocate its scratch)
    torch.cuda.synchronize()
    ev = devbuf.late_inputs(stream, [md], [real])
    ids, cnt = vg.mask_to_rows(ctx, md, rows, out=out, stream=stream)
    assert not ev.query(), "vg_mask_to_rows waited for the stream"
    stream.synchronize()
    ids = ids.cpu().numpy().view(np.uint32)
    assert cnt.cpu().tolist() == [w.size for w in want]
    for q in range(3):
        assert np.array_equal(ids[q, :want[q].size], want[q]) and (ids[q, want[q].size:] == INV).all()


@pytest.mark.parametrize("shared", [False, True])
def test_query_chunks_under_a_small_scratch_cap(vg, ctx, shared):
    """VG_PREFILTER_SMALL_SCRATCH cuts the query chunks for 64 KiB of lists and keys: 90 queries with ~300 listed rows each go in
    several chunks (ragged lists; one of them longer than a chunk's budget on its own), with the same bits as in one chunk"""
    from tests import hooks
    rng = np.random.default_rng(64)
    n, dim = 3000, 64
    c = Case(vg, ctx, rng.standard_normal((n, dim)), dim, o.METRIC_DOT)
    q = rng.standard_normal((90, dim)).astype(np.float32)
    masks = rng.random(n) < 0.1 if shared else rng.random((90, n)) < rng.choice([0.02, 0.1, 0.2], 90)[:, None]
    if not shared:
        masks[41] = True          # 3000 rows x 12 bytes: more than the whole budget, a chunk of its own
    one = c.check(q, 10, masks, "one chunk")
    hooks.set_hook("VG_PREFILTER_SMALL_SCRATCH", 1)
    try:
        many = c.check(q, 10, masks, "one chunk")
        c.check(q, 70, masks, "one chunk")
    finally:
        hooks.set_hook("VG_PREFILTER_SMALL_SCRATCH", 0)
    assert np.array_equal(one[0], many[0]) and np.array_equal(bits(one[1]), bits(many[1]))
