"""vg_search_flat above 128 queries nominates on the split tile (flat_gemm_split_big_kernel: the fp32 rows split into bfloat16
hi + lo at operand-read time, three bf16 matrix products per pair).  The tile only NOMINATES: every case here compares ids and
score bits with the same call under VG_FLAT_NO_SPLIT (the fp32 MFMA GEMM) and with the oracle's flat scan, and reads
profile_read("flat_split_launches") to know which of the two ran."""
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests.test_flat_split_bound import adversarial_corpus

pytestmark = pytest.mark.gpu

HOOK = "VG_FLAT_NO_SPLIT"
KMAX = 64


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def launches(ctx):
    return ctx.profile_read("flat_split_launches")[0]


def both_ways(ctx, idx, search, other_hook=None):
    """search() as the library runs it and under VG_FLAT_NO_SPLIT: [(result, split launches, flat_stats delta)] of each"""
    out = []
    for on in (0, 1):
        hooks.set_hook(HOOK, on)
        if other_hook:
            hooks.set_hook(other_hook, 1)
        try:
            launches(ctx)
            s0 = idx.flat_stats()
            r = search()
            s1 = idx.flat_stats()
            out.append((r, launches(ctx), (s1[0] - s0[0], s1[1] - s0[1])))
        finally:
            hooks.set_hook(HOOK, 0)
            if other_hook:
                hooks.set_hook(other_hook, 0)
    return out


def host(x):
    return x.cpu().numpy().view(np.uint32) if hasattr(x, "cpu") else np.asarray(x).view(np.uint32)


def same(a, b, what):
    assert np.array_equal(host(a[0]), host(b[0])), (what, "ids")
    assert np.array_equal(host(a[1]), host(b[1])), (what, "score bits")


def check_oracle(res, rows, q, k, metric, which, what):
    ids, sc = res
    for i in which:
        eid, esc = o.flat_search_f32(rows, rows.shape[1], q[i], k, metric)
        assert np.array_equal(ids[i], eid), (what, i, ids[i], eid)
        assert np.array_equal(bits(sc[i]), bits(esc)), (what, i)


@functools.lru_cache(maxsize=None)
def data(dim):
    rng = np.random.default_rng(2000 + dim)
    rows = rng.standard_normal((5000, dim)).astype(np.float32)
    rows[2500] = rows[7]                        # duplicates: ties broken by row id
    rows[4098] = rows[7]
    q = rng.standard_normal((300, dim)).astype(np.float32)
    q[3] = rows[7]
    return rows, q


@functools.lru_cache(maxsize=None)
def reference(n, dim, metric):
    rows, q = data(dim)
    return {i: o.flat_search_f32(rows[:n], dim, q[i], KMAX, metric) for i in (0, 3, 128, 255, 299)}


# ---- 1. ragged tiles and K steps: dim 32 = one K step, 96 = the ring of three row tiles wraps ----------------------------
@pytest.mark.parametrize("metric", [0, 2], ids=["L2", "Dot"])
@pytest.mark.parametrize("dim", [32, 64, 96, 768])
def test_ragged_tiles_and_k_steps(vg, ctx, dim, metric):
    rows, q = data(dim)
    for n in (4097, 5000):
        exp = reference(n, dim, metric)
        idx = vg.Index(ctx, n, dim, vg.Metric(metric))
        idx.set_vectors(rows[:n])
        try:
            for nq in (129, 256, 300):
                for k in (1, 10, 64):
                    (r, ran, st), (r0, ran0, st0) = both_ways(ctx, idx, lambda: idx.search_flat(q[:nq], k))
                    assert (ran, ran0) == (1, 0), (n, nq, k, ran, ran0)
                    same(r, r0, (n, nq, k))
                    assert st[0] == st0[0] == nq
                    for i, (eid, esc) in exp.items():
                        if i < nq:
                            assert np.array_equal(r[0][i], eid[:k]), (n, nq, k, i)
                            assert np.array_equal(bits(r[1][i]), bits(esc[:k])), (n, nq, k, i)
        finally:
            idx.close()


# ---- 2. no sample (n <= 4096): thresholds +Inf, capped for the tile ---------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2], ids=["L2", "Dot"])
@pytest.mark.parametrize("n", [300, 4096])
def test_no_sample(vg, ctx, n, metric):
    rows, q = data(64)
    idx = vg.Index(ctx, n, 64, vg.Metric(metric))
    idx.set_vectors(rows[:n])
    try:
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat(q[:129], 10))
        assert (ran, ran0) == (1, 0)
        same(r, r0, n)
        check_oracle(r, rows[:n], q, 10, metric, (0, 3, 128), n)
    finally:
        idx.close()


# ---- 3. persistent stream: 4 x 385 tiles on 256 workgroups, >= 6 tiles each: the parked appends flush mid-stream ---------
def test_persistent_stream_and_flush_cadence(vg, ctx):
    n, dim, nq, k = 98305, 32, 1024, 10
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(rows)
    try:
        (r, ran, st), (r0, ran0, st0) = both_ways(ctx, idx, lambda: idx.search_flat(q, k))
        assert (ran, ran0) == (1, 0)
        same(r, r0, "stream")
        check_oracle(r, rows, q, k, 0, (0, 511, 1023), "stream")
    finally:
        idx.close()


# ---- 4. dispatch edges: where the split tile must not run -----------------------------------------------------------------
def test_dispatch_edges(vg, ctx):
    import torch
    from tests import devbuf
    rows, q = data(64)
    idx = vg.Index(ctx, 5000, 64)
    idx.set_vectors(rows)
    try:
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat(q[:128], 10))     # one 128-query tile
        assert (ran, ran0) == (0, 0)
        same(r, r0, "nq = 128")
        check_oracle(r, rows, q, 10, 0, (0, 127), "nq = 128")
        # register-staged operands (what a call without 16-byte alignment gets): no LDS-DMA, no split tile
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat(q[:129], 10), other_hook="VG_FLAT_NO_DMA")
        assert (ran, ran0) == (0, 0)
        same(r, r0, "no dma")
        check_oracle(r, rows, q, 10, 0, (0, 128), "no dma")
        # a device query tensor 4 bytes off 16-byte alignment: the library stages it into an aligned block (DESIGN.md "Alignment"),
        # so the tile runs — on the staged copy — and the answer is the aligned call's
        qd = devbuf.offset_like(q[:129], 4)
        ctx.profile_read("staged_device_buffers")
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat(qd, 10))
        torch.cuda.synchronize()
        assert ctx.profile_read("staged_device_buffers")[0] >= 2 and (ran, ran0) == (1, 0)
        same(r, r0, "offset")
        check_oracle((r[0].cpu().numpy().view(np.uint32), r[1].cpu().numpy()), rows, q, 10, 0, (0, 128), "offset")
    finally:
        idx.close()
    rng = np.random.default_rng(48)                                                              # dim % 32 != 0
    rows48, q48 = rng.standard_normal((5000, 48)).astype(np.float32), rng.standard_normal((129, 48)).astype(np.float32)
    idx = vg.Index(ctx, 5000, 48)
    idx.set_vectors(rows48)
    try:
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat(q48, 10))
        assert (ran, ran0) == (0, 0)
        same(r, r0, "dim 48")
        check_oracle(r, rows48, q48, 10, 0, (0, 128), "dim 48")
    finally:
        idx.close()


# ---- 5. near-ties: more rows within the margin of the k-th than the 64 candidates ----------------------------------------
def test_near_ties_fall_back(vg, ctx):
    n, dim, nq, k = 5000, 64, 129, 10
    rng = np.random.default_rng(5)
    centre = rng.standard_normal(dim).astype(np.float32)
    rows = (3.0 * rng.standard_normal((n, dim))).astype(np.float32)
    rows[100:300] = (centre + 1e-4 * rng.standard_normal((200, dim))).astype(np.float32)   # 200 rows, distances^2 ~ 1e-6 apart
    q = (centre + 1e-4 * rng.standard_normal((nq, dim))).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(rows)
    try:
        (r, ran, st), (r0, ran0, st0) = both_ways(ctx, idx, lambda: idx.search_flat(q, k))
        assert (ran, ran0) == (1, 0)
        assert st[0] == nq and st[1] > 0, st            # the proof cannot hold: the exhaustive kernel did the work
        same(r, r0, "near ties")
        check_oracle(r, rows, q, k, 0, (0, 64, 128), "near ties")
    finally:
        idx.close()


# ---- 6. the CPU test's adversarial corpus: the split loses the most on the three nearest rows ------------------------------
def test_adversarial_corpus(vg, ctx):
    rows, query, near = adversarial_corpus()
    q = np.tile(query, (129, 1))
    idx = vg.Index(ctx, rows.shape[0], rows.shape[1])
    idx.set_vectors(rows)
    try:
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat(q, 10))
        assert (ran, ran0) == (1, 0)
        same(r, r0, "adversarial")
        assert all(r[0][i, :3].tolist() == near for i in range(129))
        check_oracle(r, rows, q, 10, 0, (0, 128), "adversarial")
    finally:
        idx.close()


# ---- 7. values the split cannot represent ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2], ids=["L2", "Dot"])
def test_non_finite_rows(vg, ctx, metric):
    n, dim, nq, k = 1000, 32, 129, 10
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[5, 3] = np.inf
    rows[40, 0] = np.nan
    rows[300, 31] = np.float32(3.3e38)          # finite in fp32, its bfloat16 hi half is Inf
    rows[301, 7] = np.float32(1e-40)            # denormal
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(rows)
    try:
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat(q, k))
        assert (ran, ran0) == (1, 0)
        same(r, r0, "non-finite")
        for i in (0, 64, 128):
            eid, esc = o.flat_search_f32(rows, dim, q[i], k, metric)
            assert np.array_equal(r[0][i], eid), (i, r[0][i], eid)
            assert np.array_equal(r[1][i], esc, equal_nan=True), i
    finally:
        idx.close()


# ---- 8. a row filter --------------------------------------------------------------------------------------------------------
def test_filter_bitmap(vg, ctx):
    rows, q = data(64)
    n, nq, k = 5000, 129, 10
    keep = np.arange(n) % 2 == 0
    idx = vg.Index(ctx, n, 64)
    idx.set_vectors(rows)
    try:
        (r, ran, _), (r0, ran0, _) = both_ways(ctx, idx, lambda: idx.search_flat_filtered(q[:nq], k, keep))
        assert (ran, ran0) == (1, 0)
        same(r, r0, "filter")
        sub = np.flatnonzero(keep)
        for i in (0, 3, 128):
            eid, esc = o.flat_search_f32(rows[keep], 64, q[i], k, 0)
            assert np.array_equal(r[0][i], sub[eid]), i
            assert np.array_equal(bits(r[1][i]), bits(esc)), i
    finally:
        idx.close()


# ---- 9. the caller's stream -------------------------------------------------------------------------------------------------
def test_callers_stream(vg, ctx):
    import torch
    rows, q = data(64)
    idx = vg.Index(ctx, 5000, 64)
    idx.set_vectors(rows)
    try:
        want = idx.search_flat(q[:129], 10)
        s = torch.cuda.Stream()
        qd = torch.from_numpy(q[:129]).cuda()
        torch.cuda.synchronize()
        launches(ctx)
        with torch.cuda.stream(s):
            ids, sc = idx.search_flat(qd, 10, stream=s)
        s.synchronize()
        assert launches(ctx) == 1
        assert np.array_equal(ids.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(bits(sc.cpu().numpy()), bits(want[1]))
    finally:
        idx.close()
