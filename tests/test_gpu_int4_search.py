"""vg_search_int4: the exhaustive top-k search over an index's INT4 codes, against tests/int4_search_ref.py — per-row scores
from the oracle's Int4Quantizer.l2_distance (the precomputed-table order), the rows that take part offered in ascending order to
the reference's CandidateHeap (ReplaceTop).  Ids compared exactly, scores by bit pattern, padding slots included.  The shapes
are the smallest at which each piece can go wrong: every row-loop form the dispatch picks and its seams, the query-block seams
of the multi-query kernel, pages beyond 64 results across a tie run longer than a page, several trips per wave and several
lists per merge (VG_INT4_SEARCH_SMALL_GRID), every mask form, NaN scores, and agreement with the calls that score the same
rows (the DiskANN walk with INT4 scoring, the distance batch)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as o
from tests import devbuf, hooks
from tests import int4_search_ref as ref

pytestmark = pytest.mark.gpu

QB = ref.QB
INV = ref.INVALID_ID


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


class Data:
    """rows, their quantizer (device and oracle), codes, an index with the codes, queries, and the oracle's row scores per query
    (computed once, on demand, and left unchanged)"""

    def __init__(self, vg, ctx, n, dim, nq, seed, ties=False, params=None):
        rng = np.random.default_rng(seed)
        self.n, self.dim, self.nq = n, dim, nq
        x = (rng.standard_normal((n, dim)) * (rng.random(dim) * 2 + 0.25)).astype(np.float32)
        if ties:
            x[10:91] = x[5]    # rows 10..90 identical to row 5: a run of 81 ties, longer than a page of 64
        self.x = x
        self.iq = vg.Int4Quantizer(ctx, dim)
        self.ref = o.Int4Quantizer(dim)
        self.iq.train(x)
        self.ref.train(x)
        self.codes = self.iq.encode(x)     # (the codes come from the trained parameters; `params` only changes the scoring)
        if params is not None:
            self.iq.set_params(*params)
            self.ref.set_params(*params)
        self.q = (rng.standard_normal((nq, dim)) * 1.5).astype(np.float32)
        if ties:
            self.q[0] = x[5]
        self.idx = vg.Index(ctx, n, dim)
        self.idx.set_int4_codes(self.iq, self.codes)
        self._scores = {}

    def scores(self, qi):
        if qi not in self._scores:
            self._scores[qi] = ref.row_scores(self.ref, self.q[qi], self.codes)
        return self._scores[qi]

    def check(self, ids, sc, k, queries=None, mask=None, what=""):
        """mask: None, bool [n] for the batch, or bool [nq, n]"""
        for qi in (range(self.nq) if queries is None else queries):
            m = None if mask is None else (mask if mask.ndim == 1 else mask[qi])
            wid, wsc = ref.expected(self.scores(qi), k, m)
            ref.assert_row(devbuf.to_host(ids)[qi], devbuf.to_host(sc)[qi], wid, wsc, (what, "query", qi))


def sub_index(vg, ctx, d, n):
    """an index over the first n rows of d (the same quantizer)"""
    idx = vg.Index(ctx, n, d.dim)
    idx.set_int4_codes(d.iq, d.codes[:n])
    return idx


def path_of(dim, nq):
    """the kernel a shape is meant to take (vg_profile_read names)"""
    if nq > QB and dim % 32 == 0:
        return "int4_search_mq"
    return "int4_search_one" if dim % 64 == 0 else "int4_search_row"


PATHS = ("int4_search_one", "int4_search_mq", "int4_search_row")


def taken(ctx):
    return {p for p in PATHS if ctx.profile_read(p)[0] > 0}


# one 32-block; one 64-block; dim % 64 != 0; one whole 128-byte piece; a short last piece; the table form's ceiling and just
# past it; dim % 32 != 0; an odd dim with a half-used last byte
DISPATCH_DIMS = [32, 64, 96, 256, 320, 768, 1024, 1536, 100, 33]


@pytest.mark.parametrize("dim", DISPATCH_DIMS)
def test_row_dispatch(vg, ctx, dim):
    d = Data(vg, ctx, 1000, dim, QB + 1, seed=dim)
    ctx.profile_enable(True)
    try:
        for n in (1, 63, 64, 65, 1000):
            idx = d.idx if n == d.n else sub_index(vg, ctx, d, n)
            for nq in (1, QB + 1):
                for p in PATHS:
                    ctx.profile_read(p)
                ids, sc = idx.search_int4(d.q[:nq], 10)
                assert taken(ctx) == {path_of(dim, nq)}, (n, nq)
                for qi in (range(nq) if n < 1000 else ref.spread(nq, 1)):
                    wid, wsc = ref.expected(d.scores(qi)[:n], 10)
                    ref.assert_row(ids[qi], sc[qi], wid, wsc, (dim, n, nq, qi))
    finally:
        ctx.profile_enable(False)


def test_every_path_is_taken(vg, ctx):
    """the three path names, each by the shape meant to take it"""
    ctx.profile_enable(True)
    try:
        seen = {}
        for dim, nq in ((64, 1), (32, QB + 1), (33, 1)):
            d = Data(vg, ctx, 130, dim, nq, seed=7 * dim)
            for p in PATHS:
                ctx.profile_read(p)
            ids, sc = d.idx.search_int4(d.q, 5)
            seen[(dim, nq)] = taken(ctx)
            d.check(ids, sc, 5)
        assert seen == {(64, 1): {"int4_search_one"}, (32, QB + 1): {"int4_search_mq"}, (33, 1): {"int4_search_row"}}
    finally:
        ctx.profile_enable(False)


@pytest.fixture(scope="module")
def d128(vg, ctx):
    return Data(vg, ctx, 3000, 128, 130, seed=128, ties=True)


@pytest.fixture(scope="module")
def d768(vg, ctx):
    return Data(vg, ctx, 700, 768, 3, seed=768, ties=True)


@pytest.mark.parametrize("nq", [1, 2, QB - 1, QB, QB + 1, 2 * QB + 1, 130])
def test_query_block_seams(d128, nq):
    ids, sc = d128.idx.search_int4(d128.q[:nq], 10)
    d128.check(ids, sc, 10, ref.spread(nq))


@pytest.mark.parametrize("k", [1, 64, 65, 128, 300, 512])
def test_selection_and_pages(d128, d768, k):
    """k > 64 comes in pages of 64, each after the previous page's last key; query 0 equals row 5 and its 81 copies"""
    for d, nqs in ((d128, (1, 3)), (d768, (1, 3))):
        for nq in nqs:
            ids, sc = d.idx.search_int4(d.q[:nq], k)
            d.check(ids, sc, k, range(nq), what=(d.dim, k, nq))
    if k >= 128:   # the tie run sits at the head of query 0's list, in row order, across the page seam
        ids, sc = d128.idx.search_int4(d128.q[:1], k)
        assert ids[0, :82].tolist() == [5] + list(range(10, 91))


def test_fewer_rows_than_k_and_k_limit(vg, ctx, d128):
    idx = sub_index(vg, ctx, d128, 50)
    for nq in (1, 3):
        ids, sc = idx.search_int4(d128.q[:nq], 64)
        for qi in range(nq):
            wid, wsc = ref.expected(d128.scores(qi)[:50], 64)
            assert np.all(wid[50:] == INV)
            ref.assert_row(ids[qi], sc[qi], wid, wsc, (nq, qi))
    with pytest.raises(vg.VecgoHipError) as e:
        d128.idx.search_int4(d128.q[:1], 513)
    assert e.value.status == -5 and "513" in str(e.value)


@pytest.mark.parametrize("dim", [256, 768])
def test_several_trips_and_lists(vg, ctx, dim):
    """VG_INT4_SEARCH_SMALL_GRID: 2 workgroups / slices, so 20 000 rows (313 tiles) give every wave several trips and the merge
    several lists; the answers are those of the full grid"""
    d = Data(vg, ctx, 20000, dim, QB + 1, seed=dim + 1)
    full = {}
    for nq in (1, QB + 1):
        for k in (10, 100):
            full[(nq, k)] = d.idx.search_int4(d.q[:nq], k)
    hooks.set_hook("VG_INT4_SEARCH_SMALL_GRID", 1)
    try:
        small = {key: d.idx.search_int4(d.q[:key[0]], key[1]) for key in full}
    finally:
        hooks.set_hook("VG_INT4_SEARCH_SMALL_GRID", 0)
    for (nq, k), (ids, sc) in full.items():
        sid, ssc = small[(nq, k)]
        assert np.array_equal(ids, sid) and np.array_equal(sc.view(np.uint32), ssc.view(np.uint32)), (nq, k)
        d.check(ids, sc, k, [0] if nq == 1 else [0, QB - 1, QB], what=(dim, nq, k))


def _masks(n, nq, rng):
    m = {}
    m["batch"] = rng.random(n) < 0.4
    m["per_query"] = rng.random((nq, n)) < 0.3
    few = np.zeros(n, bool)
    few[rng.choice(n, 6, replace=False)] = True
    m["fewer_than_k"] = few
    m["none"] = np.zeros(n, bool)
    tiles = rng.random(n) < 0.5
    for t in range(0, n, 64):
        if (t // 64) % 3 != 1:
            tiles[t:t + 64] = False     # two of every three 64-row tiles dropped whole
    m["whole_tiles"] = tiles
    pq_tiles = np.stack([np.roll(tiles, 64 * i) for i in range(nq)])
    m["whole_tiles_per_query"] = pq_tiles
    return m


@pytest.mark.parametrize("dim", [128, 768, 100])
def test_masks(vg, ctx, dim):
    n, nq, k = 1500, QB + 1, 10
    d = Data(vg, ctx, n, dim, nq, seed=3 * dim)
    rng = np.random.default_rng(dim)
    for name, m in _masks(n, nq, rng).items():
        for cnt in (1, nq):
            mm = m if m.ndim == 1 else m[:cnt]
            ids, sc = d.idx.search_int4(d.q[:cnt], k, mask=mm)
            d.check(ids, sc, k, range(cnt) if cnt == 1 else ref.spread(cnt, 1), mask=mm, what=(name, cnt))
            if name == "none":
                assert np.all(ids == INV) and np.all(np.isposinf(sc))
    # one mask per query at a stride larger than ceil(n / 8): packed rows with slack bytes (set, to be ignored) behind each
    m = rng.random((nq, n)) < 0.3
    packed = np.packbits(m, axis=-1, bitorder="little")
    wide = np.full((nq, packed.shape[1] + 5), 0xFF, np.uint8)
    wide[:, :packed.shape[1]] = packed
    ids, sc = d.idx.search_int4(d.q, k, mask=wide)
    d.check(ids, sc, k, ref.spread(nq, 1), mask=m, what="wide stride")


@pytest.mark.parametrize("dim", [64, 256, 33])
def test_mask_keeps_the_last_row_of_a_ragged_tile(vg, ctx, dim):
    d = Data(vg, ctx, 65, dim, QB + 1, seed=dim + 65)
    m = np.zeros(65, bool)
    m[64] = True
    for cnt in (1, QB + 1):
        ids, sc = d.idx.search_int4(d.q[:cnt], 4, mask=m)
        assert np.all(ids[:, 0] == 64) and np.all(ids[:, 1:] == INV)
        d.check(ids, sc, 4, range(cnt), mask=m)


def test_too_short_mask_stride_is_refused(vg, ctx, d128):
    n, nq, k = d128.n, 3, 4
    lib = ctx._lib
    q = np.ascontiguousarray(d128.q[:nq])
    mask = np.full(nq * ((n + 7) // 8), 0xFF, np.uint8)
    ids = np.full((nq, k), 77, np.uint32)
    sc = np.full((nq, k), -3.0, np.float32)
    st = lib.vg_search_int4(d128.idx._h, C.c_void_p(q.ctypes.data), C.c_int64(nq), C.c_int32(k), C.c_void_p(mask.ctypes.data),
                            C.c_int64((n + 7) // 8 - 1), C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), None)
    assert st == -1   # VG_ERR_INVALID_ARG
    assert np.all(ids == 77) and np.all(sc == -3.0)


@pytest.mark.parametrize("dim,nq", [(128, 1), (128, QB + 1), (768, 1), (100, 2)])
def test_device_buffers_at_odd_offsets_on_a_callers_stream(vg, ctx, dim, nq):
    import torch
    n, k = 900, 12
    d = Data(vg, ctx, n, dim, nq, seed=dim + nq)
    rng = np.random.default_rng(nq)
    m = rng.random((nq, n)) < 0.5 if nq > 1 else rng.random(n) < 0.5
    packed = np.packbits(m, axis=-1, bitorder="little")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dq = devbuf.offset_like(d.q, 4)
        dm = devbuf.offset_like(packed, 1)
        out_i = devbuf.offset_like(np.zeros((nq, k), np.uint32), 4)
        out_s = devbuf.offset_like(np.zeros((nq, k), np.float32), 4)
        # the inputs' producer is still running on the caller's stream when the search is enqueued behind it
        stage_q, stage_m = devbuf.whole(d.q), devbuf.whole(packed)
        devbuf.late_inputs(stream, [dq, dm], [stage_q, stage_m])
        ids, sc = d.idx.search_int4(dq, k, mask=dm, out=(out_i, out_s), stream=stream)
    stream.synchronize()
    hid = devbuf.to_host(ids).view(np.uint32).reshape(nq, k)
    hsc = devbuf.to_host(sc).reshape(nq, k)
    d.check(hid, hsc, k, range(nq), mask=m)


def _nan_queries(d):
    q = d.q.copy()
    q[0, 3] = np.nan
    q[1, d.dim - 1] = np.inf
    return q      # q[2:] all finite


@pytest.mark.parametrize("dim", [128, 768, 100])
def test_nan_queries(vg, ctx, dim):
    """a query holding a NaN, one holding +Inf and finite ones in one batch: the reference's heap, operation by operation"""
    d = Data(vg, ctx, 300, dim, 3, seed=dim + 9)
    d.q = _nan_queries(d)
    for k in (5, 70):
        ids, sc = d.idx.search_int4(d.q, k)
        d.check(ids, sc, k, what=("batch", k))
        for qi in range(3):
            i1, s1 = d.idx.search_int4(d.q[qi:qi + 1], k)
            wid, wsc = ref.expected(d.scores(qi), k)
            ref.assert_row(i1[0], s1[0], wid, wsc, ("single", qi, k))


@pytest.mark.parametrize("dim", [128, 768, 100])
def test_nan_from_the_quantizer(vg, ctx, dim):
    """diff holds an Inf in one dimension: a row whose nibble there is 0 decodes 0 * Inf = NaN and scores NaN, every other row
    decodes Inf and scores +Inf — NaN and tied +Inf scores by the row: the heap's history decides"""
    rng = np.random.default_rng(dim)
    mn = (rng.standard_normal(dim) * 0.5).astype(np.float32)
    df = (rng.random(dim) * 2 + 0.1).astype(np.float32)
    df[7] = np.inf
    d = Data(vg, ctx, 300, dim, 3, seed=dim + 11, params=(mn, df))
    sc0 = d.scores(0)
    assert not np.all(np.isfinite(sc0))
    for k in (5, 70):
        ids, sc = d.idx.search_int4(d.q, k)
        d.check(ids, sc, k, what=("batch", k))
        i1, s1 = d.idx.search_int4(d.q[:1], k)
        wid, wsc = ref.expected(sc0, k)
        ref.assert_row(i1[0], s1[0], wid, wsc, ("single", k))


def test_agrees_with_the_vamana_walk(vg, ctx):
    """every (id, score) search_vamana(kind=3) returns appears in search_int4(k = n) with the same score bits"""
    n, dim, nq, r = 400, 128, 5, 16
    d = Data(vg, ctx, n, dim, nq, seed=400)
    rng = np.random.default_rng(1)
    g = np.stack([rng.choice(n, r, replace=False) for _ in range(n)]).astype(np.uint32)
    d.idx.set_vamana_graph(g, 0)
    wid, wsc = d.idx.search_vamana(d.q, 10, kind=3)
    ids, sc = d.idx.search_int4(d.q, n)
    for qi in range(nq):
        score_of = {int(i): s for i, s in zip(ids[qi], sc[qi].view(np.uint32))}
        for i, s in zip(wid[qi], wsc[qi].view(np.uint32)):
            if i != INV:
                assert score_of[int(i)] == s, (qi, i)
        assert np.count_nonzero(wid[qi] != INV) > 0


@pytest.mark.parametrize("n,dim", [(400, 128), (512, 768), (300, 100)])
def test_scores_equal_the_distance_batch(vg, ctx, n, dim):
    """k = n <= 512: every row's score is the GPU's own precomputed-order distance for that row"""
    d = Data(vg, ctx, n, dim, 2, seed=n + dim)
    for nq in (1, 2):
        ids, sc = d.idx.search_int4(d.q[:nq], n)
        for qi in range(nq):
            dist = d.iq.l2_distance(d.q[qi], d.codes)
            assert sorted(ids[qi].tolist()) == list(range(n))
            assert np.array_equal(sc[qi].view(np.uint32), np.asarray(dist, np.float32)[ids[qi]].view(np.uint32))


def test_refusals_and_empties(vg, ctx, d128):
    dim = 128
    q = d128.q[:2]
    bare = vg.Index(ctx, 10, dim)                 # rows, no INT4 codes
    with pytest.raises(vg.VecgoHipError) as e:
        bare.search_int4(q, 3)
    assert e.value.status == -9
    # nq = 0 and k = 0 write nothing
    lib = ctx._lib
    ids = np.full((2, 4), 77, np.uint32)
    sc = np.full((2, 4), -3.0, np.float32)
    qq = np.ascontiguousarray(q)
    for nq, k in ((0, 4), (2, 0)):
        st = lib.vg_search_int4(d128.idx._h, C.c_void_p(qq.ctypes.data), C.c_int64(nq), C.c_int32(k), None, C.c_int64(0),
                                C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data), None)
        assert st == 0
        assert np.all(ids == 77) and np.all(sc == -3.0)
    empty = vg.Index(ctx, 0, dim)
    ids, sc = empty.search_int4(q, 3)
    assert np.all(ids == INV) and np.all(np.isposinf(sc))


def test_pipeline_recall_floor(vg, ctx):
    """the reference's floor for INT4 (integration_test/quantization_recall_test.go:33-38): recall@10 >= 0.85 against exact
    fp32 L2, here for the pipeline search_int4(k = 40) -> rerank(k = 10) over 500 x 128 unit vectors, 20 unit queries"""
    rng = np.random.default_rng(42)
    x = rng.standard_normal((500, 128)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = rng.standard_normal((20, 128)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    iq = vg.Int4Quantizer(ctx, 128)
    iq.train(x)
    idx = vg.Index(ctx, 500, 128)
    idx.set_vectors(x)
    idx.set_int4_codes(iq, iq.encode(x))
    cand, _ = idx.search_int4(q, 40)
    ids, _ = idx.rerank(q, cand, 10)
    d2 = ((q[:, None, :].astype(np.float64) - x[None, :, :].astype(np.float64)) ** 2).sum(-1)
    truth = np.argsort(d2, axis=1, kind="stable")[:, :10]
    recall = np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / 10.0 for i in range(20)])
    print("INT4 scan + rerank recall@10:", recall)
    assert recall >= 0.85
