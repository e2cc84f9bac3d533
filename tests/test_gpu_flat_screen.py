"""vg_search_flat above 128 queries, k <= 16: a one-product bfloat16 SCREEN (flat_gemm_screen_big_kernel, q_hi.x_hi with the
bfloat16 rounding in the proof's margin) in front of the split tile, which then runs only on the 256-query tiles that hold a query
whose screen proof failed.  Every case runs three ways — as the library runs it, under VG_FLAT_NO_SCREEN (the split tile for every
tile, no screen) and under VG_FLAT_SCREEN_FAIL (every screen proof counts as failed: every query is retried) — and wants the same
ids and score bits from all three and from the oracle's flat scan; flat_retried() and flat_stats() tell which pass answered.

k = 17 .. 48: the library runs no screen there (gemm_runs_screen, k_flat.hip: with the screen on, this file's random rows had
17 of 129 queries retried at dim 32, k = 48, and 129 of 129 at dim 768 — on the GPU and in a numpy model of the proof alike: the
48th neighbour is not 2^-7 (|q|^2 + max |x|^2) below the 64th), so the default run's "0 retried" holds at k = 48 because the split
tile answers alone; VG_FLAT_SCREEN_FAIL runs the screen up to k = 48 and retries every query."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hooks
from tests.test_flat_split_bound import adversarial_corpus
from tests.test_gpu_flat_split import bits, check_oracle, data, host, launches, reference, same

pytestmark = pytest.mark.gpu

WAYS = (None, "VG_FLAT_NO_SCREEN", "VG_FLAT_SCREEN_FAIL")


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def three_ways(ctx, idx, search, ways=WAYS):
    """search() each way: {hook: (result, split launches, searched, exhaustive, retried)}; the three results must be the same"""
    out = {}
    for hook in ways:
        if hook:
            hooks.set_hook(hook, 1)
        try:
            launches(ctx)
            s0, r0 = idx.flat_stats(), idx.flat_retried()
            r = search()
            s1, r1 = idx.flat_stats(), idx.flat_retried()
            out[hook] = (r, launches(ctx), s1[0] - s0[0], s1[1] - s0[1], r1 - r0)
        finally:
            if hook:
                hooks.set_hook(hook, 0)
    for hook in ways[1:]:
        same(out[ways[0]][0], out[hook][0], hook)
    return out


def counters(out):
    return {hook: v[1:] for hook, v in out.items()}


# ---- 1. random rows: the screen proves every query; ragged tiles, one K step (dim 32), the wrapping ring (dim 96) -----------
@pytest.mark.parametrize("metric", [0, 2], ids=["L2", "Dot"])
@pytest.mark.parametrize("dim", [32, 64, 96, 768])
def test_random_rows(vg, ctx, dim, metric):
    rows, q = data(dim)
    for n in (4097, 5000):
        exp = reference(n, dim, metric)
        idx = vg.Index(ctx, n, dim, vg.Metric(metric))
        idx.set_vectors(rows[:n])
        try:
            for nq in (129, 256, 257, 300):               # 257: a second query tile that holds a single query
                for k in (1, 10, 48):
                    out = three_ways(ctx, idx, lambda: idx.search_flat(q[:nq], k))
                    assert counters(out) == {None: (1, nq, 0, 0), "VG_FLAT_NO_SCREEN": (1, nq, 0, 0),
                                             "VG_FLAT_SCREEN_FAIL": (1, nq, 0, nq)}, (n, nq, k, counters(out))
                    r = out[None][0]
                    for i, (eid, esc) in exp.items():
                        if i < nq:
                            assert np.array_equal(r[0][i], eid[:k]), (n, nq, k, i)
                            assert np.array_equal(bits(r[1][i]), bits(esc[:k])), (n, nq, k, i)
        finally:
            idx.close()


def test_dispatch(vg, ctx):
    """k = 49 .. 64 keep the split tile alone, k = 17 .. 48 unless VG_FLAT_SCREEN_FAIL asks for the screen; VG_FLAT_NO_SPLIT
    turns the screen off with the split tile"""
    rows, q = data(64)
    idx = vg.Index(ctx, 5000, 64)
    idx.set_vectors(rows)
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat(q[:129], 49))
        assert counters(out) == {w: (1, 129, 0, 0) for w in WAYS}, counters(out)
        for k in (16, 17):
            out = three_ways(ctx, idx, lambda: idx.search_flat(q[:129], k))
            assert counters(out) == {None: (1, 129, 0, 0), "VG_FLAT_NO_SCREEN": (1, 129, 0, 0), "VG_FLAT_SCREEN_FAIL": (1, 129, 0, 129)}, (k, counters(out))
            check_oracle(out[None][0], rows, q, k, 0, (0, 128), k)
        hooks.set_hook("VG_FLAT_NO_SPLIT", 1)
        try:
            out = three_ways(ctx, idx, lambda: idx.search_flat(q[:129], 10))
        finally:
            hooks.set_hook("VG_FLAT_NO_SPLIT", 0)
        assert counters(out) == {w: (0, 129, 0, 0) for w in WAYS}, counters(out)
        check_oracle(out[None][0], rows, q, 10, 0, (0, 128), "no split")
    finally:
        idx.close()


# ---- 2. no sample (n <= 4096): thresholds capped, every row appended -----------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2], ids=["L2", "Dot"])
@pytest.mark.parametrize("n", [300, 4096])
def test_no_sample(vg, ctx, n, metric):
    rows, q = data(64)
    idx = vg.Index(ctx, n, 64, vg.Metric(metric))
    idx.set_vectors(rows[:n])
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat(q[:129], 10))
        c = counters(out)
        assert c == {None: (1, 129, 0, 0), "VG_FLAT_NO_SCREEN": (1, 129, 0, 0), "VG_FLAT_SCREEN_FAIL": (1, 129, 0, 129)}, c
        check_oracle(out[None][0], rows[:n], q, 10, metric, (0, 3, 128), n)
    finally:
        idx.close()


# ---- 3. partial retry: a gap between the 10th and the 65th neighbour that lies between the two margins -----------------------
def clustered(dim, spread, at):
    """5000 rows of which 300 (1000 .. 1299, outside the sampled tile) lie around a centre c at squared distances evenly spaced
    over (0, spread]; 600 queries, those of `at` equal to c.  For them the 10th-to-65th gap is spread * 55 / 300."""
    rng = np.random.default_rng(7000 + dim)
    rows = data(dim)[0].copy()
    c = rng.standard_normal(dim).astype(np.float32)
    u = rng.standard_normal((300, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rows[1000:1300] = (c + np.sqrt(spread * np.arange(1, 301) / 300.0)[:, None] * u).astype(np.float32)
    q = rng.standard_normal((600, dim)).astype(np.float32)
    q[list(at)] = c
    return rows, q


@pytest.mark.parametrize("at", [(5, 130, 255), (520,)], ids=["tile0", "tile2"])
@pytest.mark.parametrize("dim,spread", [(32, 0.3), (96, 1.0), (768, 30.0)])
def test_partial_retry_skips_the_other_tiles(vg, ctx, dim, spread, at):
    rows, q = clustered(dim, spread, at)
    idx = vg.Index(ctx, 5000, dim)
    idx.set_vectors(rows)
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat(q, 10))
        c = counters(out)
        print(f"partial retry dim={dim} at={at}: (launches, searched, exhaustive, retried) = {c}")
        assert c[None] == (1, 600, 0, len(at)), c                    # exactly the queries at the centre, proved by the split tile
        assert c["VG_FLAT_NO_SCREEN"] == (1, 600, 0, 0) and c["VG_FLAT_SCREEN_FAIL"] == (1, 600, 0, 600), c
        check_oracle(out[None][0], rows, q, 10, 0, tuple(at) + (0, 256, 599), "partial retry")
    finally:
        idx.close()


# ---- 4. both proofs fail: the exhaustive kernel answers ---------------------------------------------------------------------
def test_adversarial_corpus_falls_through(vg, ctx):
    rows, query, near = adversarial_corpus()
    q = np.tile(query, (129, 1))
    idx = vg.Index(ctx, rows.shape[0], rows.shape[1])
    idx.set_vectors(rows)
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat(q, 10))
        c = counters(out)
        print(f"adversarial corpus: (launches, searched, exhaustive, retried) = {c}")
        assert c[None][3] > 0 and c[None][2] > 0, c
        assert c[None][2] == c["VG_FLAT_NO_SCREEN"][2] == c["VG_FLAT_SCREEN_FAIL"][2], c
        r = out[None][0]
        assert all(r[0][i, :3].tolist() == near for i in range(129))
        check_oracle(r, rows, q, 10, 0, (0, 128), "adversarial")
    finally:
        idx.close()


def test_near_ties_fall_through(vg, ctx):
    """tests/test_gpu_flat_split.py test_near_ties_fall_back's data: 200 rows within 1e-6 of each other around the queries"""
    n, dim, nq, k = 5000, 64, 129, 10
    rng = np.random.default_rng(5)
    centre = rng.standard_normal(dim).astype(np.float32)
    rows = (3.0 * rng.standard_normal((n, dim))).astype(np.float32)
    rows[100:300] = (centre + 1e-4 * rng.standard_normal((200, dim))).astype(np.float32)
    q = (centre + 1e-4 * rng.standard_normal((nq, dim))).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(rows)
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat(q, k))
        c = counters(out)
        print(f"near ties: (launches, searched, exhaustive, retried) = {c}")
        assert c[None][3] > 0 and c[None][2] > 0, c
        assert c[None][2] == c["VG_FLAT_NO_SCREEN"][2] == c["VG_FLAT_SCREEN_FAIL"][2], c
        check_oracle(out[None][0], rows, q, k, 0, (0, 64, 128), "near ties")
    finally:
        idx.close()


# ---- 5. the split tile's other cases, once each -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2], ids=["L2", "Dot"])
def test_non_finite_rows(vg, ctx, metric):
    n, dim, nq, k = 1000, 32, 129, 10
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[5, 3] = np.inf
    rows[40, 0] = np.nan
    rows[300, 31] = np.float32(3.3e38)          # finite in fp32, its bfloat16 half is Inf
    rows[301, 7] = np.float32(1e-40)            # denormal
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim, vg.Metric(metric))
    idx.set_vectors(rows)
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat(q, k))
        c = counters(out)
        assert c[None][3] == nq and c[None][2] == nq, c       # max |x|^2 is not finite: no proof holds, one wasted pass
        r = out[None][0]
        for i in (0, 64, 128):
            eid, esc = o.flat_search_f32(rows, dim, q[i], k, metric)
            assert np.array_equal(r[0][i], eid), (i, r[0][i], eid)
            assert np.array_equal(r[1][i], esc, equal_nan=True), i
    finally:
        idx.close()


def test_filter_bitmap(vg, ctx):
    rows, q = data(64)
    n, nq, k = 5000, 129, 10
    keep = np.arange(n) % 2 == 0
    idx = vg.Index(ctx, n, 64)
    idx.set_vectors(rows)
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat_filtered(q[:nq], k, keep))
        assert counters(out) == {None: (1, nq, 0, 0), "VG_FLAT_NO_SCREEN": (1, nq, 0, 0), "VG_FLAT_SCREEN_FAIL": (1, nq, 0, nq)}, counters(out)
        r = out[None][0]
        sub = np.flatnonzero(keep)
        for i in (0, 3, 128):
            eid, esc = o.flat_search_f32(rows[keep], 64, q[i], k, 0)
            assert np.array_equal(r[0][i], sub[eid]), i
            assert np.array_equal(bits(r[1][i]), bits(esc)), i
    finally:
        idx.close()


def test_callers_stream_and_odd_offset(vg, ctx):
    import torch
    from tests import devbuf
    rows, q = data(64)
    idx = vg.Index(ctx, 5000, 64)
    idx.set_vectors(rows)
    try:
        want = idx.search_flat(q[:129], 10)
        s = torch.cuda.Stream()
        qd = torch.from_numpy(q[:129]).cuda()
        torch.cuda.synchronize()

        def on_stream():
            with torch.cuda.stream(s):
                ids, sc = idx.search_flat(qd, 10, stream=s)
            s.synchronize()
            return ids, sc
        out = three_ways(ctx, idx, on_stream)
        assert counters(out)["VG_FLAT_SCREEN_FAIL"] == (1, 129, 0, 129) and counters(out)[None] == (1, 129, 0, 0), counters(out)
        same(out[None][0], want, "stream / offset")
        # a device query tensor 4 bytes off 16-byte alignment: staged into an aligned block, then the same cascade
        qo = devbuf.offset_like(q[:129], 4)
        out = three_ways(ctx, idx, lambda: idx.search_flat(qo, 10))
        torch.cuda.synchronize()
        assert counters(out)["VG_FLAT_SCREEN_FAIL"] == (1, 129, 0, 129) and counters(out)[None] == (1, 129, 0, 0), counters(out)
        same(out[None][0], want, "stream / offset")
    finally:
        idx.close()


# ---- 6. persistent stream: 4 x 385 tiles on 256 workgroups — the screen's and (SCREEN_FAIL) the split tile's flush cadence ----
def test_persistent_stream(vg, ctx):
    n, dim, nq, k = 98305, 32, 1024, 10
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(rows)
    try:
        out = three_ways(ctx, idx, lambda: idx.search_flat(q, k))
        assert counters(out) == {None: (1, nq, 0, 0), "VG_FLAT_NO_SCREEN": (1, nq, 0, 0), "VG_FLAT_SCREEN_FAIL": (1, nq, 0, nq)}, counters(out)
        check_oracle(out[None][0], rows, q, k, 0, (0, 511, 1023), "stream")
    finally:
        idx.close()
