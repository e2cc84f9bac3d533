"""vg_search_binary: the exhaustive Hamming top-k over an index's binary codes, against numpy — np.unpackbits of the xor,
np.lexsort on (row, h), padded to k.  Ids equal, scores equal as float32.  Codes are BinaryQuantizer.encode's; the queries'
bits are numpy's (v >= threshold).  The shapes: every query-block size and its ragged last block, one 8-byte word to two stage
pieces (dim 1536) and the 8-byte-load form (dim 1088: 17 words), ragged tiles, k past a page of 64 and past the rows, a tie run
over every row (dim 8), and the same under VG_BINARY_SMALL_GRID (2 workgroups: several trips a wave, several lists a merge).
The matrix-core path (VG_BINARY_NOM_ALWAYS) against the reference and the scan: every row listed (300 rows), the sampled
threshold (more than 64 tiles), ragged query and row tiles, lists that overflow on ties, and the batches it must not take."""
import numpy as np
import pytest

from tests import devbuf, hooks

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
NOT_READY, UNSUPPORTED = -9, -5


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


_data = {}


def data(vg, ctx, n, dim, nq):
    """(quantizer, codes, queries, rows' Hamming distances [nq, n], an index holding the codes): made once per shape"""
    if (n, dim, nq) not in _data:
        rng = np.random.default_rng(n * 7 + dim * 3 + nq)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        bq = vg.BinaryQuantizer(ctx, dim)
        bq.train(x)
        codes = np.asarray(bq.encode(x))
        qc = np.zeros((nq, codes.shape[1]), np.uint8)
        bits = np.packbits(q >= bq.threshold, axis=1, bitorder="little")
        qc[:, :bits.shape[1]] = bits
        h = np.stack([np.unpackbits(codes ^ c, axis=1).sum(1) for c in qc])
        idx = vg.Index(ctx, n, dim)
        idx.set_binary_codes(bq, codes)
        _data[(n, dim, nq)] = (bq, codes, q, h, idx)
    return _data[(n, dim, nq)]


def expected(h, k, mask=None):
    """h [nq, n]; mask None, bool [n] or bool [nq, n]"""
    ids = np.full((len(h), k), INV, np.uint32)
    sc = np.full((len(h), k), np.inf, np.float32)
    for qi, hq in enumerate(h):
        rows = np.arange(len(hq)) if mask is None else np.flatnonzero(mask if mask.ndim == 1 else mask[qi])
        best = rows[np.lexsort((rows, hq[rows]))][:k]
        ids[qi, :len(best)] = best
        sc[qi, :len(best)] = hq[best]
    return ids, sc


def assert_equal(got, want):
    ids, sc = devbuf.to_host(got[0]).view(np.uint32).reshape(want[0].shape), devbuf.to_host(got[1]).reshape(want[1].shape)
    np.testing.assert_array_equal(ids, want[0])
    np.testing.assert_array_equal(sc, want[1])


# (dim, rows, nq, k): every dim, row count, batch size and k of the scan's list in at least one case; k > rows; dim 8 over 5000
# rows (at most 9 distinct scores: the order is the row id's); 17 words (the 8-byte loads)
SCAN = [(1, 63, 1, 1), (64, 257, 4, 10), (65, 5000, 5, 64), (100, 257, 9, 65), (128, 1, 33, 10), (192, 5000, 33, 512),
        (768, 5000, 9, 10), (768, 63, 1, 512), (768, 5000, 1, 65), (1536, 257, 5, 65), (1536, 5000, 4, 1), (8, 5000, 4, 64),
        (1088, 257, 5, 10)]


@pytest.mark.parametrize("small_grid", [0, 1])
@pytest.mark.parametrize("dim,n,nq,k", SCAN)
def test_scan(vg, ctx, dim, n, nq, k, small_grid):
    bq, codes, q, h, idx = data(vg, ctx, n, dim, nq)
    hooks.set_hook("VG_BINARY_NO_NOM", 1)
    hooks.set_hook("VG_BINARY_SMALL_GRID", small_grid)
    try:
        got = idx.search_binary(q, k)
    finally:
        hooks.set_hook("VG_BINARY_SMALL_GRID", 0)
        hooks.set_hook("VG_BINARY_NO_NOM", 0)
    assert_equal(got, expected(h, k))
    assert idx.binary_info()[0] == (n + 63) // 64 * 64 * codes.shape[1]


def test_device_buffers_at_odd_offsets_on_a_callers_stream(vg, ctx):
    import torch
    n, dim, nq, k = 900, 192, 9, 12
    bq, codes, q, h, _ = data(vg, ctx, n, dim, nq)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dc, dq = devbuf.offset_like(codes, 1), devbuf.offset_like(q, 4)
        out = devbuf.offset_like(np.zeros((nq, k), np.uint32), 4), devbuf.offset_like(np.zeros((nq, k), np.float32), 4)
        # the inputs' producer is still running on the caller's stream when the calls are enqueued behind it
        devbuf.late_inputs(stream, [dc, dq], [devbuf.whole(codes), devbuf.whole(q)])
        idx = vg.Index(ctx, n, dim)
        idx.set_binary_codes(bq, dc, stream=stream)
        got = idx.search_binary(dq, k, out=out, stream=stream)
    stream.synchronize()
    assert_equal(got, expected(h, k))


# nq 9: a ragged block of 16; 4 and 1: the 4- and 1-query kernels (one query's mask is always the batch's)
@pytest.mark.parametrize("nq", [9, 4, 1])
@pytest.mark.parametrize("form", ["batch_tenth", "per_query", "fewer_than_k", "empty_tiles"])
def test_masks(vg, ctx, form, nq):
    n, dim, k = 5000, 192, 10
    bq, codes, q, h, idx = data(vg, ctx, n, dim, nq)
    rng = np.random.default_rng(len(form))
    if form == "batch_tenth":
        m = rng.random(n) < 0.1
    elif form == "per_query":
        m = rng.random((nq, n) if nq > 1 else n) < 0.3
    elif form == "fewer_than_k":
        m = np.zeros(n, bool)
        m[[3, 64, 4097, 4999]] = True
    else:
        m = np.zeros(n, bool)
        m[128:200] = m[4992:] = True    # tiles 2 and 3 (the second ragged inside) and the last, ragged one
    assert_equal(idx.search_binary(q, k, mask=m), expected(h, k, m))


def nominated(idx, q, k, **kw):
    """search_binary under VG_BINARY_NOM_ALWAYS: the result and how binary_info()'s (nominated, rescanned) moved"""
    before = idx.binary_info()
    hooks.set_hook("VG_BINARY_NOM_ALWAYS", 1)
    try:
        got = idx.search_binary(q, k, **kw)
    finally:
        hooks.set_hook("VG_BINARY_NOM_ALWAYS", 0)
    after = idx.binary_info()
    return got, after[1] - before[1], after[2] - before[2]


# (nq, rows, dim, k): 300 rows: no sample, every row listed; 4097 and 20000: the sampled seam at more than 64 tiles
MATRIX = [(129, 300, 100, 1), (256, 4097, 128, 10), (257, 20000, 192, 256), (129, 20000, 768, 10), (257, 300, 768, 256),
          (256, 20000, 100, 1), (129, 4097, 192, 256), (257, 4097, 768, 1), (256, 300, 128, 10)]


@pytest.mark.parametrize("nq,n,dim,k", MATRIX)
def test_matrix_path(vg, ctx, nq, n, dim, k):
    bq, codes, q, h, idx = data(vg, ctx, n, dim, nq)
    got, took, rescanned = nominated(idx, q, k)
    print("rescanned", rescanned, "of", nq)
    assert took == nq and 0 <= rescanned <= nq
    assert_equal(got, expected(h, k))
    hooks.set_hook("VG_BINARY_NO_NOM", 1)
    try:
        scan = idx.search_binary(q, k)
    finally:
        hooks.set_hook("VG_BINARY_NO_NOM", 0)
    assert_equal(got, (np.asarray(scan[0]).view(np.uint32), np.asarray(scan[1])))


def test_matrix_path_ties_end_in_the_scan(vg, ctx):
    """5000 identical rows: every list overflows, every query is the scan's, the answer is rows 0 .. k-1 at one distance"""
    n, dim, nq, k = 5000, 128, 129, 10
    bq, _, q, _, _ = data(vg, ctx, 300, dim, nq)
    codes = np.repeat(np.asarray(bq.encode(q[:1])), n, axis=0)
    idx = vg.Index(ctx, n, dim)
    idx.set_binary_codes(bq, codes)
    (ids, sc), took, rescanned = nominated(idx, q, k)
    assert took == nq and rescanned == nq
    assert np.all(np.asarray(ids).view(np.uint32) == np.arange(k, dtype=np.uint32))
    assert np.all(sc == sc[:, :1]) and np.all(sc[0] == 0)


@pytest.mark.parametrize("why", ["mask", "k300"])
def test_matrix_path_not_taken(vg, ctx, why):
    n, dim, nq = 4097, 128, 256
    bq, codes, q, h, idx = data(vg, ctx, n, dim, nq)
    m = np.ones(n, bool) if why == "mask" else None
    k = 10 if why == "mask" else 300
    got, took, rescanned = nominated(idx, q, k, mask=m)
    assert (took, rescanned) == (0, 0)
    assert_equal(got, expected(h, k, m))


def test_state_and_refusals(vg, ctx):
    n, dim = 40, 64
    bq, codes, q, h, _ = data(vg, ctx, n, dim, 2)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n + 2, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_binary(q, 3)
    assert e.value.status == NOT_READY and "binary codes" in e.value.message
    idx.set_binary_codes(bq, codes)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_binary(q, 513)
    assert e.value.status == UNSUPPORTED
    assert_equal(idx.search_binary(q, 3), expected(h, 3))
    idx.set_binary_codes(bq, None)      # dropped
    assert idx.binary_info() == (0, 0, 0)
    with pytest.raises(vg.VecgoHipError) as e:
        idx.search_binary(q, 3)
    assert e.value.status == NOT_READY
    # an index holding binary codes is a segment's: what appends or moves rows refuses it until the codes are dropped
    idx.set_vectors(x[:n])
    idx.build_hnsw(m=8, ef_construction=32)
    ring = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + 2) % n], axis=1).astype(np.uint32)
    vam = vg.Index(ctx, n, dim)
    vam.set_vectors(x[:n])
    vam.set_vamana_graph(ring, 0)
    for index, call in ((idx, lambda: idx.insert_hnsw(x[n:], m=8, ef_construction=32)), (vam, vam.reorder_vamana_bfs)):
        index.set_binary_codes(bq, codes)
        with pytest.raises(vg.VecgoHipError) as e:
            call()
        assert e.value.status == UNSUPPORTED and "binary codes" in e.value.message
        index.set_binary_codes(bq, None)
        call()
