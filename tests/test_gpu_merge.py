"""vg_index_merge and vecgo_amd.compact on the GPU against Engine.CompactWithContext's Iterate loop restated in numpy
(tests/compact_ref.py), against a freshly uploaded index of the same rows, and against the builders' separate calls:
every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from tests import compact_ref as ref
from tests import flat_writer_ref as fref

pytestmark = pytest.mark.gpu

INVALID = ref.INVALID
KERNELS = ("merge_count", "merge_scan", "merge_rank", "merge_gather")


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def upload(vg, ctx, x, metric=0):
    idx = vg.Index(ctx, len(x), x.shape[1], vg.Metric(metric))
    idx.set_vectors(x)
    return idx


def pack(dead):
    return np.packbits(np.asarray(dead, bool), bitorder="little")


def check_merge(vg, ctx, idxs, xs, deleted, given=None, metric=0, stream=None):
    """merge `idxs` under `given` (what the call is handed; default: `deleted`, the host bitmaps) and compare the maps and
    the merged index's rows with the helper's; returns the merged index and the helper's rows"""
    dim = xs[0].shape[1]
    merged, o2n, ns, nr = vg.merge_indexes(ctx, idxs, deleted if given is None else given, stream=stream)
    rows, want_o2n, want_ns, want_nr = ref.merge(xs, deleted)
    assert o2n.dtype == np.uint32 and ns.dtype == np.int32 and nr.dtype == np.uint32
    assert np.array_equal(o2n, want_o2n)
    assert np.array_equal(ns, want_ns) and np.array_equal(nr, want_nr)
    assert merged.n == len(rows) and merged.dim == dim
    assert merged.write_flat_segment(3) == fref.image(3, rows, dim, metric, checksum=vg.crc32c)
    return merged, rows


# ---- 1. the loop itself --------------------------------------------------------------------------------------------------
def _loop_cases():
    """name, sizes, dim, deleted(rng, sizes) -> list of bool arrays / None, or None"""
    def rand(p):
        return lambda rng, sizes: [rng.random(n) < p for n in sizes]

    def run_of_blocks(rng, sizes):      # rows 256 .. 5000: whole 2048-row work blocks without a live row
        d = np.zeros(sizes[0], bool)
        d[256:5001] = True
        return [d]

    def ends(rng, sizes):
        out = []
        for n in sizes:
            d = np.zeros(n, bool)
            d[0] = d[-1] = True
            out.append(d)
        return out

    def middle(rng, sizes):
        return [rng.random(sizes[0]) < 0.2, np.ones(sizes[1], bool), None]

    yield "identity", [1000], 8, None
    yield "empty and one-row sources", [257, 0, 4099, 1], 8, rand(0.3)
    yield "carry across many workgroups", [70001], 4, rand(0.5)
    for dim in (1, 3, 6, 4):            # 4-byte words (odd dim), 8-byte words (dim 6), 16-byte words (dim 4)
        yield f"two sources at dim {dim}", [20011, 20011], dim, rand(0.3)
    yield "whole work blocks deleted", [9000], 8, run_of_blocks
    yield "first and last row deleted", [5000, 2048, 1], 8, ends
    yield "a middle source fully deleted", [3000, 2500, 100], 8, middle
    yield "every source fully deleted", [300, 2049], 8, rand(1.1)
    yield "a wide row", [700, 300], 200, rand(0.3)   # 50 sixteen-byte words: 64 lanes per row, some idle


@pytest.mark.parametrize("name,sizes,dim,deleted", list(_loop_cases()), ids=[c[0] for c in _loop_cases()])
def test_loop(vg, ctx, name, sizes, dim, deleted):
    rng = np.random.default_rng(sum(sizes) + dim)
    xs = [rng.standard_normal((n, dim)).astype(np.float32) for n in sizes]
    idxs = [upload(vg, ctx, x) for x in xs]
    dead = None if deleted is None else [None if d is None else pack(d) for d in deleted(rng, sizes)]
    merged, rows = check_merge(vg, ctx, idxs, xs, dead)
    if name == "every source fully deleted":
        assert merged.n == 0 and merged.flat_build(4)[0].size == 0      # an index of 0 rows, as vg_index_create(n = 0) leaves
    if name == "identity":
        assert np.array_equal(rows, xs[0])


def test_high_bits_of_the_last_byte(vg, ctx):
    rng = np.random.default_rng(7)
    sizes = [13, 2051, 8]
    xs = [rng.standard_normal((n, 8)).astype(np.float32) for n in sizes]
    idxs = [upload(vg, ctx, x) for x in xs]
    dead = []
    for n in sizes:
        b = pack(rng.random(n) < 0.3)
        if n % 8:
            b[-1] |= (0xFF << (n % 8)) & 0xFF       # bits at or above n: not rows
        dead.append(b)
    assert dead[0][-1] >> 5 == 7 and dead[1][-1] >> 3 == 31
    merged, _ = check_merge(vg, ctx, idxs, xs, dead)
    assert merged.n == sum(int((~ref.unpack(b, n)).sum()) for b, n in zip(dead, sizes))


def test_many_sources_and_launch_count(vg, ctx):
    """37 sources of 0 .. 3000 rows; and (4.) the merge's kernels are launched as often for 37 sources as for one"""
    rng = np.random.default_rng(37)
    sizes = [int(n) for n in rng.integers(0, 3001, 37)]
    sizes[0], sizes[5] = 2500, 0
    xs = [rng.standard_normal((n, 8)).astype(np.float32) for n in sizes]
    idxs = [upload(vg, ctx, x) for x in xs]
    dead = [pack(rng.random(n) < 0.3) for n in sizes]
    dead[11] = None
    ctx.profile_enable(True)
    try:
        for k in KERNELS:
            ctx.profile_read(k)
        check_merge(vg, ctx, idxs[:1], xs[:1], dead[:1])
        one = [ctx.profile_read(k)[0] for k in KERNELS]
        check_merge(vg, ctx, idxs, xs, dead)
        many = [ctx.profile_read(k)[0] for k in KERNELS]
    finally:
        ctx.profile_enable(False)
    assert one == many == [1, 1, 1, 1], (one, many)


def test_the_same_source_twice(vg, ctx):
    rng = np.random.default_rng(2)
    a, b = (rng.standard_normal((n, 8)).astype(np.float32) for n in (3001, 700))
    ia, ib = upload(vg, ctx, a), upload(vg, ctx, b)
    dead = [pack(rng.random(3001) < 0.5), None, pack(rng.random(3001) < 0.1)]     # each listing under its own bitmap
    merged, rows = check_merge(vg, ctx, [ia, ib, ia], [a, b, a], dead)
    assert merged.n > 3001 + 700


def test_device_bitmaps_at_odd_offsets_and_the_callers_stream(vg, ctx):
    import torch

    from tests import devbuf
    rng = np.random.default_rng(9)
    sizes = [4100, 2049, 515, 64]
    xs = [rng.standard_normal((n, 8)).astype(np.float32) for n in sizes]
    idxs = [upload(vg, ctx, x) for x in xs]
    host = [pack(rng.random(n) < 0.4) for n in sizes]
    # device buffers one byte into their allocation, one left on the host, one absent
    given = [devbuf.offset_like(host[0], 1), host[1], devbuf.offset_like(host[2], 1), None]
    assert given[0].data_ptr() % 2 == 1
    check_merge(vg, ctx, idxs, xs, [host[0], host[1], host[2], None], given=given)
    # the caller's own stream: the bitmaps hold 0xFF (everything deleted) until a copy late on that stream fills them in
    stream = torch.cuda.Stream()
    late = [devbuf.offset_like(np.zeros_like(h), 1) for h in host]
    real = [devbuf.whole(h) for h in host]
    torch.cuda.synchronize()
    devbuf.late_inputs(stream, late, real)
    merged, _ = check_merge(vg, ctx, idxs, xs, host, given=late, stream=stream)
    assert merged.n > 0
    torch.cuda.synchronize()


# ---- 2. the merged index is the index a host would have uploaded -------------------------------------------------------------
def test_merged_index_searches_like_a_fresh_upload(vg, ctx):
    rng = np.random.default_rng(21)
    dim, sizes = 64, [6000, 5000, 4000]
    xs = [rng.standard_normal((n, dim)).astype(np.float32) for n in sizes]
    xs[1][1234] *= np.float32(np.sqrt(1000.0))          # one row with 10^3 times the others' norm ...
    dead = [rng.random(n) < 0.25 for n in sizes]
    dead[1][1234] = True                                # ... deleted: it may hold source 1's largest norm, not the result's
    kept = [d.copy() for d in dead]
    kept[1][1234] = False
    idxs = [upload(vg, ctx, x) for x in xs]
    merged, rows = check_merge(vg, ctx, idxs, xs, [pack(d) for d in dead])
    fresh = upload(vg, ctx, rows)
    with_outlier = upload(vg, ctx, ref.merge(xs, kept)[0])
    q12 = rng.standard_normal((12, dim)).astype(np.float32)
    q200 = rng.standard_normal((200, dim)).astype(np.float32)      # above 128 queries: the split tile (dim % 32 == 0)
    for q in (q12, q200):
        got, want = merged.search_flat(q, 10), fresh.search_flat(q, 10)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
        with_outlier.search_flat(q, 10)
    cand = rng.integers(0, merged.n, (12, 40)).astype(np.uint32)
    got, want = merged.rerank(q12, cand, 5), fresh.rerank(q12, cand, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    stats, want_stats, outlier_stats = merged.flat_stats(), fresh.flat_stats(), with_outlier.flat_stats()
    print(f"flat_stats (queries, exhaustive): merged {stats}, fresh {want_stats}, fresh with the outlier kept {outlier_stats}")
    # the outlier is visible at this shape: kept, its norm widens the nomination's error bound and sends queries to the
    # exhaustive kernel that the merged rows' own maximum does not — a stale d_norm_max would show as outlier_stats
    assert outlier_stats[0] == want_stats[0] and outlier_stats[1] != want_stats[1]
    assert stats == want_stats


@pytest.mark.parametrize("dim", [3, 6, 200], ids=["4-byte words", "8-byte words", "64 lanes per row"])
def test_norms_and_maxima_at_every_gather_shape(vg, ctx, dim):
    """the segment image holds rows only: the gathered norms and the two recomputed maxima are what the searches read, so
    the merged index must answer, and count, like a fresh upload at every word width of the gather"""
    rng = np.random.default_rng(dim)
    sizes = [3001, 0, 2050]
    xs = [rng.standard_normal((n, dim)).astype(np.float32) for n in sizes]
    xs[2][77] *= np.float32(np.sqrt(1000.0))            # a deleted row that holds source 2's largest norm and largest |x|
    dead = [rng.random(n) < 0.3 for n in sizes]
    dead[2][77] = True
    idxs = [upload(vg, ctx, x) for x in xs]
    merged, rows = check_merge(vg, ctx, idxs, xs, [pack(d) for d in dead])
    fresh = upload(vg, ctx, rows)
    q12 = rng.standard_normal((12, dim)).astype(np.float32)
    q200 = rng.standard_normal((200, dim)).astype(np.float32)
    for q in (q12, q200):
        got, want = merged.search_flat(q, 10), fresh.search_flat(q, 10)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    cand = rng.integers(0, merged.n, (12, 40)).astype(np.uint32)
    got, want = merged.rerank(q12, cand, 5), fresh.rerank(q12, cand, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert merged.flat_stats() == fresh.flat_stats()


def test_device_maps_and_null_maps(vg, ctx):
    """the maps of the C entry point: each NULL to skip, host or device (the Python binding always passes host arrays)"""
    import torch

    from tests import devbuf
    rng = np.random.default_rng(17)
    sizes = [2500, 1, 4099]
    xs = [rng.standard_normal((n, 8)).astype(np.float32) for n in sizes]
    idxs = [upload(vg, ctx, x) for x in xs]
    dead = [pack(rng.random(n) < 0.3) for n in sizes]
    rows, want_o2n, want_ns, want_nr = ref.merge(xs, dead)
    total, live = sum(sizes), len(rows)
    lib = ctx._lib
    handles = (C.c_void_p * 3)(*[i._h.value for i in idxs])
    bitmaps = (C.c_void_p * 3)(*[d.ctypes.data for d in dead])

    def call(o2n, ns, nr):
        out = C.c_void_p()
        ptrs = [None if t is None else C.c_void_p(t.data_ptr()) for t in (o2n, ns, nr)]
        torch.cuda.synchronize()            # the maps' fill is done before the library's own stream writes them
        assert lib.vg_index_merge(ctx._h, handles, bitmaps, C.c_int32(3), C.byref(out), *ptrs, None) == 0
        torch.cuda.synchronize()
        merged = vg.Index._adopted(ctx, out, live, 8, 0)        # (no getter for n: counted from the bitmaps)
        assert merged.write_flat_segment(3) == fref.image(3, rows, 8, 0, checksum=vg.crc32c)
        return merged

    def dev(n, skew):
        t = np.full(n, 7, np.int32)
        return devbuf.offset_like(t, 4) if skew else devbuf.whole(t)
    for skew in (False, True):              # whole allocations, and views one element into theirs (not 16-byte aligned)
        o2n, ns, nr = dev(total, skew), dev(live + 3, skew), dev(live + 3, skew)
        call(o2n, ns, nr)
        assert np.array_equal(devbuf.to_host(o2n).view(np.uint32), want_o2n)
        assert np.array_equal(devbuf.to_host(ns)[:live], want_ns) and np.array_equal(devbuf.to_host(nr)[:live].view(np.uint32), want_nr)
        assert np.all(devbuf.to_host(ns)[live:] == 7) and np.all(devbuf.to_host(nr)[live:] == 7)     # one entry per live row, no more
    call(None, None, None)
    nr = dev(live, False)
    call(None, None, nr)                    # one map alone
    assert np.array_equal(devbuf.to_host(nr).view(np.uint32), want_nr)
    o2n = dev(total, False)
    call(o2n, None, None)
    assert np.array_equal(devbuf.to_host(o2n).view(np.uint32), want_o2n)


# ---- 3. sources are untouched --------------------------------------------------------------------------------------------
def test_sources_are_untouched(vg, ctx):
    rng = np.random.default_rng(31)
    dim = 16
    xa = rng.standard_normal((3000, dim)).astype(np.float32)
    xb = rng.standard_normal((1200, dim)).astype(np.float32)
    a, b = upload(vg, ctx, xa), upload(vg, ctx, xb)
    sq = vg.ScalarQuantizer(ctx, dim)
    perm_a, _ = a.flat_build(4, sq, seed=1)                         # partitions + SQ8 codes
    pq = vg.ProductQuantizer(ctx, dim, 4, 256)
    perm_b, _, used = b.diskann_build(8, 20, 1.2, pq, seed=2)       # a Vamana graph + PQ codes
    assert used == b.QUANT_PQ
    q = rng.standard_normal((6, dim)).astype(np.float32)

    def state():
        sa, sb = a.search_sq8(q, 5), b.search_vamana(q, 5, 1)
        return (a.write_flat_segment(1), b.write_diskann_segment(2), sa[0].tobytes(), bits(sa[1]).tobytes(), sb[0].tobytes(),
                bits(sb[1]).tobytes())
    before = state()
    dead = [pack(rng.random(3000) < 0.3), pack(rng.random(1200) < 0.3)]
    merged, rows = check_merge(vg, ctx, [a, b], [xa[perm_a], xb[perm_b]], dead)
    assert fref.parse_header(merged.write_flat_segment(3))["num_partitions"] == 0       # nothing carried over
    assert state() == before


# ---- 5. refusals on a device ---------------------------------------------------------------------------------------------
def test_refusals(vg, ctx):
    rng = np.random.default_rng(41)
    lib = ctx._lib
    x8 = rng.standard_normal((500, 8)).astype(np.float32)
    a = upload(vg, ctx, x8)
    other_dim = upload(vg, ctx, rng.standard_normal((50, 4)).astype(np.float32))
    other_metric = upload(vg, ctx, x8[:50], metric=2)
    no_rows = vg.Index(ctx, 10, 8)
    hamming = [vg.Index(ctx, 10, 8, vg.Metric.HAMMING) for _ in range(2)]
    ctx2 = vg.Context(0)
    elsewhere = upload(vg, ctx2, x8[:50])
    q = rng.standard_normal((3, 8)).astype(np.float32)
    before = a.search_flat(q, 4)

    def status(idxs, n=None):
        handles = (C.c_void_p * max(len(idxs), 1))(*[i._h.value for i in idxs])
        out = C.c_void_p(0x1234)
        maps = [np.full(600, 7, np.uint32), np.full(600, 7, np.int32), np.full(600, 7, np.uint32)]
        st = lib.vg_index_merge(ctx._h, handles, None, C.c_int32(len(idxs) if n is None else n), C.byref(out),
                                *[C.c_void_p(m.ctypes.data) for m in maps], None)
        assert out.value is None and all(np.all(m == 7) for m in maps)
        after = a.search_flat(q, 4)
        assert np.array_equal(after[0], before[0]) and np.array_equal(bits(after[1]), bits(before[1]))
        return st
    assert status([a, other_dim]) == -2                    # VG_ERR_DIM_MISMATCH
    assert status([a, other_metric]) == -1                 # VG_ERR_INVALID_ARG
    assert status([a, no_rows]) == -9                      # VG_ERR_NOT_READY
    assert status(hamming) == -5                           # VG_ERR_UNSUPPORTED (before the rows are asked for)
    assert status([a], n=0) == -1
    assert status([a, elsewhere]) == -1 and b"another context" in lib.vg_last_error()
    assert status([a, elsewhere, other_dim]) == -1         # the order: the context before the dim
    assert status([other_dim, a, other_metric]) == -2      # the dim before the metric
    with pytest.raises(vg.VecgoHipError) as e:
        vg.merge_indexes(ctx, [a, other_dim])
    assert e.value.status == -2
    elsewhere.close()
    ctx2.close()


# ---- 6. compact ----------------------------------------------------------------------------------------------------------
def _compact_sources(vg, ctx, rng, sizes, dim, p):
    xs = [rng.standard_normal((n, dim)).astype(np.float32) for n in sizes]
    return xs, [upload(vg, ctx, x) for x in xs], [pack(rng.random(n) < p) for n in sizes]


@pytest.mark.parametrize("quant", ["none", "sq8"])
def test_compact_flat(vg, ctx, quant):
    rng = np.random.default_rng(61)
    dim, seed = 8, 5
    xs, idxs, dead = _compact_sources(vg, ctx, rng, [9000, 5000, 3000], dim, 0.2)      # 17000 rows: k = 2
    assert vg.compaction_plan(17000, 100000) == ref.plan(17000, 100000) == ("flat", 2)
    quantizer = {"none": lambda: None, "sq8": lambda: vg.ScalarQuantizer(ctx, dim)}[quant]
    built, kind, o2n, ns, nr = vg.compact(ctx, idxs, dead, diskann_threshold=100000, flat_quantizer=quantizer(), seed=seed)
    rows, mo, ms, mr = ref.merge(xs, dead)
    hand = upload(vg, ctx, rows)
    perm, inv = hand.flat_build(2, quantizer(), seed=seed)
    assert kind == "flat" and not np.array_equal(perm, np.arange(len(rows)))
    image = built.write_flat_segment(4)
    assert image == hand.write_flat_segment(4)
    h = fref.parse_header(image)
    assert h["num_partitions"] == 2 and h["rows"] == len(rows) and h["quant"] == (fref.QUANT_SQ8 if quant == "sq8" else fref.QUANT_NONE)
    want = ref.compose(mo, ms, mr, perm, inv)
    assert np.array_equal(o2n, want[0]) and np.array_equal(ns, want[1]) and np.array_equal(nr, want[2])
    # the maps say where the rows are: final row j holds row nr[j] of source ns[j]
    final_rows = np.frombuffer(image, "<f4", len(rows) * dim, h["vector_off"]).reshape(-1, dim)
    assert np.array_equal(bits(final_rows), bits(np.stack([xs[s][r] for s, r in zip(ns, nr)])))


def test_compact_flat_with_fewer_live_rows_than_partitions(vg, ctx):
    rng = np.random.default_rng(62)
    dim = 8
    xs = [rng.standard_normal((n, dim)).astype(np.float32) for n in (9000, 8000)]        # 17000 rows: k = 2
    idxs = [upload(vg, ctx, x) for x in xs]
    dead = [np.ones(9000, bool), np.ones(8000, bool)]
    dead[1][4321] = False                                                                # one live row
    built, kind, o2n, ns, nr = vg.compact(ctx, idxs, [pack(d) for d in dead], diskann_threshold=100000, seed=1)
    assert kind == "flat" and built.n == 1
    assert built.write_flat_segment(4) == fref.image(4, xs[1][4321:4322], dim, 0, checksum=vg.crc32c)       # unpartitioned
    assert list(ns) == [1] and list(nr) == [4321] and o2n[9000 + 4321] == 0 and np.count_nonzero(o2n != INVALID) == 1


@pytest.mark.parametrize("p,name", [(0.1, "live rows above the threshold"), (0.5, "live rows below it, total rows above")])
def test_compact_diskann(vg, ctx, p, name):
    rng = np.random.default_rng(63)
    dim, seed = 16, 9
    xs, idxs, dead = _compact_sources(vg, ctx, rng, [1500, 1000], dim, p)                # 2500 rows, threshold 2000
    rows, mo, ms, mr = ref.merge(xs, dead)
    assert (len(rows) < 2000) == (p == 0.5) and ref.plan(2500, 2000) == ("diskann", 0)
    built, kind, o2n, ns, nr = vg.compact(ctx, idxs, dead, diskann_threshold=2000, diskann=dict(r=8, l=20), seed=seed)
    hand = upload(vg, ctx, rows)
    perm, inv, _ = hand.diskann_build(8, 20, seed=seed)
    assert kind == "diskann"
    assert built.write_diskann_segment(6, 20) == hand.write_diskann_segment(6, 20)
    want = ref.compose(mo, ms, mr, perm, inv)
    assert np.array_equal(o2n, want[0]) and np.array_equal(ns, want[1]) and np.array_equal(nr, want[2])


def test_compact_diskann_without_a_live_row_is_the_writers_refusal(vg, ctx):
    rng = np.random.default_rng(64)
    xs, idxs, _ = _compact_sources(vg, ctx, rng, [40, 30], 16, 0.0)
    with pytest.raises(vg.VecgoHipError) as e:       # "no vectors to write" (diskann/writer.go:218-220)
        vg.compact(ctx, idxs, [pack(np.ones(40, bool)), pack(np.ones(30, bool))], diskann_threshold=50, diskann=dict(r=8, l=20))
    assert e.value.status == -1
