"""vg_filter_evaluate / vg_columns_* / vg_mask_*: metadata filters evaluated on the device, against the numpy restatement
of the semantics (tests/filter_ref.py).  The check is exact: a mask is bits and a count is an integer.  The shapes are the
smallest at which the kernel can still go wrong: tails inside a byte, a 64-row word and a row tile (T rows per workgroup),
query counts around the waves' split, clause counts 0..16, every compare at the float seams."""
import ctypes as C

import numpy as np
import pytest

from tests import filter_ref as ref

pytestmark = pytest.mark.gpu

INV = ref.INVALID_ID
UNSUPPORTED, INVALID_ARG = -5, -1


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def device_columns(vg, ctx, rc: ref.RefColumns, present_none=()):
    """the library's twin of a RefColumns; fields in present_none are uploaded with present = NULL"""
    cols = vg.Columns(ctx, rc.rows)
    for field, col in rc.cols.items():
        if col[0] == "f64":
            cols.set_f64(field, col[1], None if field in present_none else col[2])
        else:
            cols.set_codes(field, col[1])
    return cols


def evaluate(vg, cols, fsets, deleted=None, **kw):
    """(masks uint8[nq, ceil(rows / 8)], counts) on the host, through the default path: clauses on the host, masks and counts on
    the device"""
    out, cnt = vg.evaluate_filters(cols, fsets, deleted=deleted, **kw)
    nbytes = (cols.rows + 7) // 8
    return out.cpu().numpy()[:, :nbytes], cnt.cpu().numpy()


def check(vg, cols, rc, fsets, deleted=None, what=None):
    want_m, want_c = ref.evaluate(rc, fsets, deleted)
    got_m, got_c = evaluate(vg, cols, fsets, deleted)
    assert got_m.shape == want_m.shape, what
    bad = np.flatnonzero((got_m != want_m).any(axis=1))
    assert bad.size == 0, (what, "queries", bad[:8].tolist(), fsets[bad[0]])
    assert np.array_equal(got_c, want_c), what
    return want_m, want_c


def status_of(vg, fn):
    with pytest.raises(vg.VecgoHipError) as e:
        fn()
    return e.value.status, e.value.message


def three_kinds(rng, rows):
    """two f64 fields (the second partly absent) and a code field"""
    rc = ref.RefColumns(rows)
    rc.set_f64(0, rng.random(rows))
    rc.set_f64(1, rng.integers(0, 20, rows).astype(np.float64), rng.random(rows) < 0.8)
    codes = rng.integers(0, 6, rows).astype(np.uint32)
    codes[rng.random(rows) < 0.1] = INV
    rc.set_codes(2, codes)
    return rc


# ---- row seams ---------------------------------------------------------------------------------------------------------------
def _row_seams():
    import vecgo_amd
    t = vecgo_amd.FILTER_TILE_ROWS
    return [1, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, t - 1, t, t + 1, 2 * t + 37]


@pytest.mark.parametrize("rows", sorted(set(_row_seams())))
def test_row_seams_and_guard_bytes(vg, ctx, rows):
    import torch
    rng = np.random.default_rng(rows)
    rc = three_kinds(rng, rows)
    cols = device_columns(vg, ctx, rc)
    deleted = rng.random(rows) < 0.2
    fsets = [[(0, "lt", 0.6)], [], [(1, "gte", 5.0), (2, "in", [1, 2, 5]), (0, "ne", 2.0)]]
    want_m, want_c = check(vg, cols, rc, fsets, deleted, rows)
    assert want_c[1] == rows - deleted.sum()                       # the empty set: every row that is not deleted
    nbytes = (rows + 7) // 8
    if rows % 8:
        assert not (want_m[:, -1] >> (rows % 8)).any()             # tail bits of the last byte are zero
    # guard bytes behind each query's ceil(rows / 8) bytes stay: word stores (8-aligned stride), byte stores (odd stride), host
    for stride in ((nbytes + 7) // 8 * 8 + 8, nbytes + 11 + (nbytes % 2)):
        for host in (False, True):
            out = np.full((3, stride), 0xA5, np.uint8)
            if not host:
                out = torch.from_numpy(out).cuda()
            got, cnt = vg.evaluate_filters(cols, fsets, deleted=deleted, out=out)
            got = got.cpu().numpy() if not host else got
            assert np.array_equal(got[:, :nbytes], want_m), (rows, stride, host)
            assert (got[:, nbytes:] == 0xA5).all(), (rows, stride, host)
            assert np.array_equal(cnt.cpu().numpy() if not host else cnt, want_c)
    cols.close()


# ---- query seams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 130])
def test_query_seams_and_clause_counts(vg, ctx, nq):
    rows = 777
    rng = np.random.default_rng(nq)
    rc = three_kinds(rng, rows)
    cols = device_columns(vg, ctx, rc)
    pool = [lambda: (0, "gt", float(rng.random() * 0.3)), lambda: (1, "lte", float(rng.integers(8, 20))),
            lambda: (2, "in", rng.integers(0, 6, 4).tolist()), lambda: (0, "ne", 0.5), lambda: (1, "ne", 3.0),
            lambda: (2, "eq", int(rng.integers(0, 6)))]
    fsets = []
    for q in range(nq):
        n = (q * 5 + nq) % 17                                       # 0 .. 16 clauses, a different count from query to query
        fields = pool[q % 2::2] if q % 3 else pool                  # neighbouring queries name different fields
        fsets.append([fields[i % len(fields)]() for i in range(n)])
    if nq > 20:
        assert {len(f) for f in fsets} >= {0, 16}
        fsets[7] = [(9, "eq", 1.0)]                                 # a field without a column: nothing
    _, want_c = check(vg, cols, rc, fsets, None, nq)
    if nq > 20:
        assert want_c[7] == 0
    cols.close()


def test_seventeen_clauses_are_refused(vg, ctx):
    rc = three_kinds(np.random.default_rng(1), 100)
    cols = device_columns(vg, ctx, rc)
    ok = [(0, "ne", 0.5)] * 16
    check(vg, cols, rc, [ok], None, "16 clauses")
    st, msg = status_of(vg, lambda: vg.evaluate_filters(cols, [ok, ok + [(0, "ne", 0.5)]]))
    assert st == UNSUPPORTED and "17" in msg
    cols.close()


# ---- compare seams -----------------------------------------------------------------------------------------------------------
SPECIALS = [-0.0, 0.0, np.inf, -np.inf, np.nan, 5e-324, 2.0 ** 53, 2.0 ** 53 + 2, -1.0, np.nextafter(1.0, 2.0), 1.0]


def test_compare_seams_every_op(vg, ctx):
    rows = 3 * 64 + 29
    values = np.array([SPECIALS[i % len(SPECIALS)] for i in range(rows)], np.float64)
    present = (np.arange(rows) // 37) % 2 == 0                       # runs of 37 rows: they cross the 64-row words
    present[60:70] = True
    present[126:130] = False
    rc = ref.RefColumns(rows)
    rc.set_f64(0, values, present)
    rc.set_f64(1, values)                                             # present = NULL: every row
    cols = device_columns(vg, ctx, rc, present_none=(1,))
    stored = [v for v in SPECIALS if not np.isnan(v)]
    operands = list(SPECIALS)
    for v in stored:
        operands += [np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]
    for field in (0, 1):
        for op in ("eq", "ne", "lt", "lte", "gt", "gte"):
            check(vg, cols, rc, [[(field, op, float(c))] for c in operands], None, (field, op))
    # gt and gte differ by exactly the equal rows; ne skips absent rows and keeps a stored NaN
    m = lambda op, c: np.unpackbits(evaluate(vg, cols, [[(0, op, c)]])[0][0], bitorder="little")[:rows].astype(bool)
    for c in stored:
        with np.errstate(invalid="ignore"):
            assert np.array_equal(m("gte", c) & ~m("gt", c), present & (values == c))
    ne = m("ne", 1.0)
    assert not ne[~present].any() and ne[present & np.isnan(values)].all()
    assert np.array_equal(m("ne", np.nan), present) and not m("eq", np.nan).any()
    cols.close()


# ---- code columns ------------------------------------------------------------------------------------------------------------
def test_code_columns(vg, ctx):
    rows = 5000
    rng = np.random.default_rng(4)
    codes = rng.integers(0, 10000, rows).astype(np.uint32)
    codes[rng.random(rows) < 0.15] = INV
    codes[:4] = [7, INV, 7, 123456789]
    rc = ref.RefColumns(rows)
    rc.set_codes(0, codes)
    rc.set_f64(1, rng.random(rows))
    cols = device_columns(vg, ctx, rc)
    absent_code = 10001
    universe = rng.permutation(10000).astype(np.uint32)
    fsets = [[(0, "eq", 7)], [(0, "eq", absent_code)], [(0, "eq", INV)], [(0, "eq", 123456789)]]
    for size in (0, 1, 2, 255, 4096):
        fsets.append([(0, "in", universe[:size].tolist())])
    fsets.append([(0, "in", [7, 7, 7, int(codes[10]), 7, int(codes[10])])])                  # duplicates
    fsets.append([(0, "in", [INV, 7])])                                                     # the no-value code inside a set
    fsets.append([(0, "in", universe[:300].tolist()), (0, "in", universe[200:3000].tolist())])   # two sets, one `sets` array
    want_m, want_c = check(vg, cols, rc, fsets, None, "codes")
    assert want_c[0] >= 2 and want_c[1] == 0 and want_c[2] == 0 and want_c[3] == 1 and want_c[4] == 0
    assert want_c[8] > 1000                                                                 # the 4096-code set is a real one
    st, msg = status_of(vg, lambda: vg.evaluate_filters(cols, [[(0, "in", list(range(4097)))]]))
    assert st == UNSUPPORTED and "4097" in msg
    st, msg = status_of(vg, lambda: vg.evaluate_filters(cols, [[(0, "lt", 5)]]))
    assert st == UNSUPPORTED and "lt" in msg
    st, msg = status_of(vg, lambda: vg.evaluate_filters(cols, [[(1, "in", [1, 2])]]))
    assert st == UNSUPPORTED and "f64" in msg
    cols.close()


def test_malformed_clauses_are_refused(vg, ctx):
    rc = three_kinds(np.random.default_rng(2), 64)
    cols = device_columns(vg, ctx, rc)
    clauses, off, sets = vg.pack_filter_sets([[(0, "lt", 0.5)], [(2, "in", [1, 2])]])
    out = np.zeros((2, 8), np.uint8)

    def call(clauses=clauses, off=off, sets=sets, n_sets=None, stride=8):
        return cols._lib.vg_filter_evaluate(cols._h, C.c_void_p(clauses.ctypes.data), C.c_void_p(off.ctypes.data), C.c_int64(2),
                                            C.c_void_p(sets.ctypes.data), C.c_int64(sets.size if n_sets is None else n_sets), None,
                                            C.c_void_p(out.ctypes.data), C.c_int64(stride), None, None)
    assert call() == 0
    for field in (-1, 64):
        bad = clauses.copy(); bad["field"][0] = field
        assert call(clauses=bad) == INVALID_ARG
    bad = clauses.copy(); bad["op"][0] = 7
    assert call(clauses=bad) == INVALID_ARG
    assert call(off=np.array([0, 2, 1], np.int32)) == INVALID_ARG        # not monotone
    assert call(off=np.array([-1, 1, 2], np.int32)) == INVALID_ARG
    assert call(n_sets=1) == INVALID_ARG                                  # the set range ends outside `sets`
    bad = clauses.copy(); bad["set_begin"][1] = -1
    assert call(clauses=bad) == INVALID_ARG
    assert call(stride=7) == INVALID_ARG and call(stride=0) == INVALID_ARG   # shorter than a mask; 0 with two queries
    cols.close()


# ---- AND across kinds, deleted rows ----------------------------------------------------------------------------------------------
def test_and_across_kinds_with_deleted_at_an_odd_address(vg, ctx):
    from tests import devbuf
    rows = 4096 + 333
    rng = np.random.default_rng(6)
    rc = three_kinds(rng, rows)
    cols = device_columns(vg, ctx, rc)
    deleted = rng.random(rows) < 0.3
    fsets = [[(0, "gte", 0.25), (1, "lt", 15.0), (2, "in", [0, 1, 2, 3])], [(2, "eq", 4), (0, "lt", 0.9)], []]
    want_m, want_c = check(vg, cols, rc, fsets, deleted, "host bool deleted")
    packed = ref.pack(deleted)
    dev = devbuf.offset_like(packed, 1)
    assert dev.data_ptr() % 2 == 1
    got_m, got_c = evaluate(vg, cols, fsets, dev)
    assert np.array_equal(got_m, want_m) and np.array_equal(got_c, want_c)
    got_m, got_c = evaluate(vg, cols, fsets, packed)                   # packed bits from the host
    assert np.array_equal(got_m, want_m) and np.array_equal(got_c, want_c)
    high = packed.copy()
    high[-1] |= 0xFF << (rows % 8) & 0xFF                              # deleted bits at or above `rows` are not rows
    got_m, _ = evaluate(vg, cols, fsets, high)
    assert np.array_equal(got_m, want_m)
    cols.close()


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def test_odd_device_mask_host_buffers_and_no_counts(vg, ctx):
    import torch

    from tests import devbuf
    rows = 4096 + 77
    nbytes = (rows + 7) // 8
    rng = np.random.default_rng(8)
    rc = three_kinds(rng, rows)
    cols = device_columns(vg, ctx, rc)
    fsets = [[(0, "lt", float(rng.random()))] + ([(2, "in", [1, 3])] if q % 2 else []) for q in range(9)]
    want_m, want_c = check(vg, cols, rc, fsets, None, "aligned")
    # the device mask one byte into its allocation, with an odd stride: the byte-store twin gives the same bits
    stride = nbytes + 3 + nbytes % 2
    assert stride % 2 == 1
    view = devbuf.offset_like(np.full((9, stride), 0x5A, np.uint8), 1)
    assert view.data_ptr() % 2 == 1
    got, cnt = vg.evaluate_filters(cols, fsets, out=view)
    got = got.cpu().numpy()
    assert np.array_equal(got[:, :nbytes], want_m) and (got[:, nbytes:] == 0x5A).all()
    assert np.array_equal(cnt.cpu().numpy(), want_c)
    # mask and counts on the host
    host = np.zeros((9, nbytes), np.uint8)
    got, cnt = vg.evaluate_filters(cols, fsets, out=host)
    assert got is host and isinstance(cnt, np.ndarray) and np.array_equal(host, want_m) and np.array_equal(cnt, want_c)
    # counts = NULL
    out = torch.zeros((9, nbytes), dtype=torch.uint8, device="cuda")
    got, cnt = vg.evaluate_filters(cols, fsets, out=out, counts=False)
    assert cnt is None and np.array_equal(out.cpu().numpy(), want_m)
    # a single query with stride 0 (a 1-D mask)
    one = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    vg.evaluate_filters(cols, fsets[:1], out=one)
    assert np.array_equal(one.cpu().numpy(), want_m[0])
    cols.close()


def test_no_rows_and_no_queries(vg, ctx):
    import torch
    empty = vg.Columns(ctx, 0)
    empty.set_f64(0, np.zeros(0))
    out = torch.full((2, 8), 0x77, dtype=torch.uint8, device="cuda")
    got, cnt = vg.evaluate_filters(empty, [[(0, "lt", 1.0)], []], out=out)
    assert (out.cpu().numpy() == 0x77).all() and cnt.cpu().numpy().tolist() == [0, 0]       # rows == 0 writes no mask byte
    empty.close()
    rc = three_kinds(np.random.default_rng(3), 50)
    cols = device_columns(vg, ctx, rc)
    got, cnt = vg.evaluate_filters(cols, [])
    assert tuple(got.shape)[0] == 0 and cnt.numel() == 0                                     # nq == 0 succeeds
    assert cols._lib.vg_filter_evaluate(cols._h, None, None, C.c_int64(0), None, C.c_int64(0), None, None, C.c_int64(0), None, None) == 0
    cols.close()


def test_everything_on_the_device_on_the_callers_stream(vg, ctx):
    """clauses, offsets, sets, deleted, masks and counts in device memory, on a stream whose producer is still queued: the call
    only enqueues, and reads its inputs behind the producer"""
    import torch

    from tests import devbuf
    rows = 2 * vg.FILTER_TILE_ROWS + 5
    nbytes = (rows + 7) // 8
    rng = np.random.default_rng(10)
    rc = three_kinds(rng, rows)
    cols = device_columns(vg, ctx, rc)
    deleted = rng.random(rows) < 0.25
    fsets = [[(0, "lt", float(rng.random())), (2, "in", rng.integers(0, 6, 3).tolist())] if q % 3 else [(1, "gt", 4.0)] for q in range(20)]
    want_m, want_c = ref.evaluate(rc, fsets, deleted)
    clauses, off, sets = vg.pack_filter_sets(fsets)
    real = [torch.from_numpy(clauses.view(np.uint8).copy()).cuda(), devbuf.whole(off), devbuf.whole(sets), devbuf.whole(ref.pack(deleted))]
    late = [torch.zeros_like(t) for t in real]
    stride = (nbytes + 7) // 8 * 8
    mask = torch.zeros((20, stride), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(20, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()

    def call():
        return cols._lib.vg_filter_evaluate(cols._h, C.c_void_p(late[0].data_ptr()), C.c_void_p(late[1].data_ptr()), C.c_int64(20),
                                            C.c_void_p(late[2].data_ptr()), C.c_int64(sets.size), C.c_void_p(late[3].data_ptr()),
                                            C.c_void_p(mask.data_ptr()), C.c_int64(stride), C.c_void_p(counts.data_ptr()),
                                            C.c_void_p(stream.cuda_stream))
    with torch.cuda.stream(stream):
        for t, r in zip(late, real):
            t.copy_(r)
        assert call() == 0                # first use of this stream: its scratch exists afterwards
    stream.synchronize()
    assert np.array_equal(mask.cpu().numpy()[:, :nbytes], want_m)
    mask.zero_()
    counts.fill_(-1)
    torch.cuda.synchronize()
    ev = devbuf.late_inputs(stream, late, real)      # the inputs hold 0xFF / -1 until a copy late on the stream
    assert not ev.query()
    assert call() == 0
    waited = ev.query()
    stream.synchronize()
    assert np.array_equal(mask.cpu().numpy()[:, :nbytes], want_m) and np.array_equal(counts.cpu().numpy(), want_c)
    assert not waited, "vg_filter_evaluate waited for the stream although every buffer is on the device"
    cols.close()


# ---- several workgroups ----------------------------------------------------------------------------------------------------------
def test_several_workgroups_random_clauses(vg, ctx):
    rows, nq = 100003, 64
    rng = np.random.default_rng(12)
    rc = three_kinds(rng, rows)
    rc.set_f64(3, rng.standard_normal(rows), rng.random(rows) < 0.5)      # more columns than the kernel stages per workgroup
    rc.set_codes(4, rng.integers(0, 1000, rows).astype(np.uint32))
    cols = device_columns(vg, ctx, rc)
    ops = ("eq", "ne", "lt", "lte", "gt", "gte")

    def clause():
        f = int(rng.integers(0, 6))                                         # 5: no such column
        if f in (2, 4):
            top = 6 if f == 2 else 1000
            return (f, "in", rng.integers(0, top, int(rng.integers(0, 40))).tolist()) if rng.random() < 0.6 else (f, "eq", int(rng.integers(0, top)))
        c = float(rng.integers(0, 20)) if f == 1 else float(rng.standard_normal() if f == 3 else rng.random())
        return (f, ops[int(rng.integers(0, 6))], c)
    fsets = [[clause() for _ in range(int(rng.integers(0, 5)))] for _ in range(nq)]
    deleted = rng.random(rows) < 0.1
    _, want_c = check(vg, cols, rc, fsets, deleted, "100003 x 64")
    assert (want_c > 0).sum() > nq // 4
    cols.close()


# ---- column life cycle -----------------------------------------------------------------------------------------------------------
def test_replace_and_drop_a_column(vg, ctx):
    rows = 1000
    rng = np.random.default_rng(14)
    rc = three_kinds(rng, rows)
    cols = device_columns(vg, ctx, rc)
    fsets = [[(0, "lt", 0.5)], [(0, "eq", 3)], [(0, "lt", 0.5), (1, "gte", 2.0)]]
    check(vg, cols, rc, fsets, None, "before")
    newv = rng.random(rows)
    rc.set_f64(0, newv, rng.random(rows) < 0.5)
    cols.set_f64(0, newv, rc.cols[0][2])
    check(vg, cols, rc, fsets, None, "replaced")
    codes = rng.integers(0, 5, rows).astype(np.uint32)                  # the field set as f64, then as codes
    rc.set_codes(0, codes)
    cols.set_codes(0, codes)
    check(vg, cols, rc, [[(0, "eq", 3)], [(0, "in", [1, 2])]], None, "f64 -> codes")
    st, _ = status_of(vg, lambda: vg.evaluate_filters(cols, [[(0, "lt", 0.5)]]))
    assert st == UNSUPPORTED
    rc.drop(0)
    cols.drop(0)
    _, c = check(vg, cols, rc, [[(0, "eq", 3)], [(1, "gte", 2.0)], []], None, "dropped")
    assert c[0] == 0 and c[2] == rows
    cols.drop(0)                                                        # dropping an empty field is fine
    cols.close()


# ---- vg_mask_combine / vg_mask_popcount ------------------------------------------------------------------------------------------
NP_OPS = {"and": lambda d, s: d & s, "andnot": lambda d, s: d & ~s, "or": lambda d, s: d | s, "xor": lambda d, s: d ^ s}


@pytest.mark.parametrize("place", ["device", "device_odd", "host"])
def test_mask_combine_and_popcount(vg, ctx, place):
    import torch

    from tests import devbuf
    rng = np.random.default_rng(16)

    def put(a):
        if place == "host":
            return a.copy()
        return devbuf.offset_like(a, 1) if place == "device_odd" else torch.from_numpy(a.copy()).cuda()

    def get(x):
        return x.cpu().numpy() if place != "host" else x
    for rows in (1, 63, 64, 65, 1000):
        nbytes = (rows + 7) // 8
        for nq in (1, 5):
            for stride in (nbytes, nbytes + 8 - nbytes % 8, nbytes + 3):
                dst0 = rng.integers(0, 256, (nq, stride), dtype=np.uint8)
                src_b = rng.integers(0, 256, (nq, stride), dtype=np.uint8)
                src_1 = rng.integers(0, 256, nbytes, dtype=np.uint8)
                for op, f in NP_OPS.items():
                    for src in (src_b, src_1):                           # src_stride non-zero, and 0: one src for every query
                        d = put(dst0)
                        vg.mask_combine(ctx, op, d, put(src), rows)
                        want = dst0.copy()
                        want[:, :nbytes] = f(dst0[:, :nbytes], src[..., :nbytes])
                        assert np.array_equal(get(d), want), (rows, nq, stride, op, src.ndim)
                cnt = get(vg.mask_popcount(ctx, put(dst0), rows))
                bits = np.unpackbits(dst0[:, :nbytes], axis=1, bitorder="little")[:, :rows]
                assert cnt.dtype == np.int64 and np.array_equal(cnt, bits.sum(axis=1))
    full = np.full((2, 2), 0xFF, np.uint8)                                # bits at or above `rows` left set in the last byte
    assert get(vg.mask_popcount(ctx, put(full), 13)).tolist() == [13, 13]
    assert get(vg.mask_popcount(ctx, put(full), 16)).tolist() == [16, 16]


# ---- end to end: the masks feed the searches ---------------------------------------------------------------------------------------
def test_device_masks_feed_the_filtered_searches(vg, ctx):
    def bits(x):
        return np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x).view(np.uint32)
    rows, dim, nq, k = 2000, 32, 40, 10
    rng = np.random.default_rng(18)
    base = rng.standard_normal((rows, dim)).astype(np.float32)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    rc = three_kinds(rng, rows)
    cols = device_columns(vg, ctx, rc)
    deleted = rng.random(rows) < 0.05
    fsets = [[(0, "gte", float(rng.random() * 0.5))] + ([(2, "in", rng.integers(0, 6, 3).tolist())] if q % 4 == 0 else [])
             + ([(1, "lt", 18.0)] if q % 3 == 0 else []) for q in range(nq)]
    want_m, want_c = ref.evaluate(rc, fsets, deleted)
    dev_m, dev_c = vg.evaluate_filters(cols, fsets, deleted=deleted)
    assert dev_m.is_cuda and dev_m.stride(0) % 8 == 0
    idx = vg.Index(ctx, rows, dim)
    idx.set_vectors(base)
    # the device mask, unchanged, with its stride, against the helper's masks from the host
    a = idx.search_flat_filtered(queries, k, dev_m)
    b = idx.search_flat_filtered(queries, k, want_m)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    assert (a[0] != INV).any()
    idx.build_hnsw(m=8, ef_construction=64, max_batch=64, growth_div=16)
    a = idx.search_hnsw_brute(queries, k, idx.BRUTE_BITMAP, dev_m)
    b = idx.search_hnsw_brute(queries, k, idx.BRUTE_BITMAP, want_m)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    # counts / rows as the selectivity hint of the post-filtered walk: the same ids as with the host's value
    dev_counts = dev_c.cpu().numpy()
    assert np.array_equal(dev_counts, want_c)
    for q in range(0, nq, 8):
        a = idx.search_hnsw_filtered(queries[q:q + 1], k, 64, dev_m[q:q + 1], dev_counts[q] / rows)
        b = idx.search_hnsw_filtered(queries[q:q + 1], k, 64, want_m[q:q + 1], want_c[q] / rows)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), q
    cols.close()
