"""vg_index_enable_pq_nomination_from_codes with on = 2 (mode 3): vg_search_pq_adc batches of 5 .. 128 queries through the matrix-core
nomination on the tile of one query tile (flat_gemm_pq_small_kernel: each lane gathers its codebook entry by its row's code byte
into the matrix instruction's register) — ids and score bits equal to the table scan's, the image mode's and the oracle's.  No
tolerance anywhere.  Every parity case asserts that the small GEMM's scope ran and that the info mode is 3."""
import numpy as np
import pytest

from oracle import oracle as o
from tests.test_gpu_pq_nomination_codes import (_clustered_codes, _decoded, _mk, _queries, _random_pq, _same, bits, ctx,  # noqa: F401
                                                nominate_always, vg)                                                    # (its fixtures and helpers)

pytestmark = pytest.mark.gpu
SMALL, BIG = "pq_codes_gemm_small", "pq_codes_gemm"   # the profile scopes of the two code-gathered GEMMs


def _launches(ctx, search):
    """search()'s result and how often each of the two GEMMs ran in it"""
    ctx.profile_enable(True)
    try:
        ctx.profile_read(SMALL), ctx.profile_read(BIG)
        r = search()
        return r, ctx.profile_read(SMALL)[0], ctx.profile_read(BIG)[0]
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("n,m,nq,k", [
    (300, 1, 5, 5),         # one sub-quantizer: lane half 1 all padding; 27 padded queries; no sample; second row tile partial
    (70, 2, 32, 10),        # one full step; fewer rows than a wave's tile
    (4097, 13, 33, 10),     # odd m, unaligned rows; the first size with a sample; one query in the second block; last row tile: one row
    (700, 16, 64, 48),      # a whole 16-byte code chunk; the pick's last k
    (700, 17, 64, 48),      # one byte past it: a second chunk of one step, the reads of the last rows clamped and shifted
    (5000, 24, 96, 100),    # RB = 3; k above the pick
    (2000, 78, 128, 10),    # RB = 4 at its last m
    (2000, 80, 128, 256),   # the first m at which 128 queries split into two launches; k at the limit
    (9000, 96, 97, 10),     # the workload's m: 6 chunks of 8 steps; two launches, 64 + 33 queries
    (1500, 108, 96, 10),    # RB = 3 no longer fits: 64 + 32
    (600, 160, 70, 10),     # one block per launch; three launches
    (600, 318, 33, 10),     # the last m that fits
    (140001, 4, 40, 10)])   # 547 row tiles for at most 512 resident workgroups: the persistent loop, the prefetch across a tile's end
def test_parity_with_scan_image_and_oracle(vg, ctx, nominate_always, n, m, nq, k):
    dim = 8 * m
    rng = np.random.default_rng(n + dim + m)
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    t = 100 if n > 112 else 30
    codes[t:t + 10] = codes[t]                        # ties
    codes[t + 10], codes[t + 11], codes[n - 1] = 0, 255, 255   # the codebook's first and last entries in every sub-quantizer
    codes[t + 12, ::2], codes[t + 12, 1::2] = 0, 255
    pq, idx = _mk(vg, ctx, opq, codes, n)
    x = _decoded(opq, codes)
    q = (x[rng.integers(0, n, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.05).astype(np.float32)
    q[1] = x[t]                                       # exactly a decoded row (one of the ten tied ones)
    plain = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination(True)
    image = idx.search_pq_adc(q, k)
    idx.enable_pq_nomination_from_codes(True, small_batches=True)
    assert idx.pq_nomination_info() == (3, n * 4 + 4 + ((dim + 63) // 64 * 8) * 256 * 16)   # nothing more resident than mode 2
    got, small, big = _launches(ctx, lambda: idx.search_pq_adc(q, k))
    assert small >= 1 and big == 0, "the batch did not run the small tile"
    assert _same(plain, got) and _same(image, got)
    for i in (0, 1, nq // 2, nq - 1):
        eid, esc = o.flat_search_pq(opq, codes, q[i], k)
        assert np.array_equal(got[0][i, :eid.size], eid) and np.array_equal(bits(got[1][i, :eid.size]), bits(esc))


def test_batches_the_mode_does_not_take(vg, ctx, nominate_always):
    rng = np.random.default_rng(6)
    for n, m, nq, k, want_big in ((6000, 16, 4, 10, 0), (6000, 16, 64, 257, 0), (600, 320, 33, 10, 0), (6000, 16, 129, 10, 1)):
        opq = _random_pq(rng, 8 * m, m)
        codes = _clustered_codes(rng, n, m)
        pq, idx = _mk(vg, ctx, opq, codes, n)
        q = _queries(rng, _decoded(opq, codes), nq)
        plain = idx.search_pq_adc(q, k)
        idx.enable_pq_nomination_from_codes(True, small_batches=True)
        got, small, big = _launches(ctx, lambda: idx.search_pq_adc(q, k))
        assert small == 0 and (big >= 1) == bool(want_big), (n, m, nq, k)
        assert _same(plain, got)
    # enabled without small_batches: mode 2, and 64 queries keep the scan (idx: the 129-query case's)
    idx.enable_pq_nomination_from_codes(True)
    assert idx.pq_nomination_info()[0] == 2
    got, small, big = _launches(ctx, lambda: idx.search_pq_adc(q[:64], k))
    assert small == 0 and big == 0 and _same((plain[0][:64], plain[1][:64]), got)


def test_far_queries_and_non_finite_values(vg, ctx, nominate_always):
    """test_far_queries_and_non_finite_values's inputs (tests/test_gpu_pq_nomination_codes.py) at 40 queries: a far query, NaN / Inf
    queries, an all-zero query, then a NaN scale (norm_max = +Inf: every proof fails) — on = 2 equals off, bit for bit"""
    rng = np.random.default_rng(321)
    n, dim, m, nq, k = 12000, 128, 16, 40, 10
    opq = _random_pq(rng, dim, m)
    codes = _clustered_codes(rng, n, m)
    x = _decoded(opq, codes)
    q = (x[rng.integers(0, n, nq)] + rng.standard_normal((nq, dim)).astype(np.float32) * 0.05).astype(np.float32)
    q[2] = rng.standard_normal(dim).astype(np.float32) * 1000.0
    q[3, 5] = np.nan
    q[4, :] = np.inf
    q[5, 7] = -np.inf
    q[6] = 0.0
    for poison in (False, True):
        if poison:
            sc = np.array(opq.scales, np.float32)
            sc[3] = np.nan
            opq.set_codebooks(opq.codebooks, sc, opq.offsets)
        pq, idx = _mk(vg, ctx, opq, codes, n)
        plain = idx.search_pq_adc(q, k)
        idx.enable_pq_nomination_from_codes(True, small_batches=True)
        got, small, big = _launches(ctx, lambda: idx.search_pq_adc(q, k))
        assert small >= 1 and big == 0
        assert _same(plain, got), poison
