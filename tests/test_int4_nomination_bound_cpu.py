"""The margin of the INT4 nomination (vg_index_enable_int4_nomination; Int4Row::eps, k_int4_nominate.hip), without a GPU: a numpy
model in the manner of tests/test_sq8_nomination_codes_bound_cpu.py.  The GEMM multiplies the query image bf16(q_d * s_d), s_d =
diff_d / 15 — the only rounded operand — by the nibbles c - 8 with fp32 accumulation from (t - |x^|^2) / 2, and scores s' = t - 2 acc;
the proof needs |s' + |q|^2 - 2 q.mid - L2Distance| <= eps for every row, mid_d = min_d + 8 s_d.  Every term but the exact score (the
oracle's Int4Quantizer.l2_distance, judged in float64) is formed in fp32 as the kernels form it."""
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as o
from tests.test_sq8_nomination_codes_bound_cpu import fma32, rne_bf16, wave_sum

ROOT = Path(__file__).resolve().parent.parent
U, F = 2.0 ** -24, np.float32


def int4_eps(dim, qn, norm_max, h2):
    """Int4Row::eps, restated"""
    return (2.0 ** -8 * 1.001 + (6.0 * dim + 160.0) * U) * (qn + norm_max) + 6.0 * U * (qn + h2) + 1e-30


def test_formula_and_entry_points_are_the_librarys():
    src = (ROOT / "vecgo_amd" / "csrc" / "k_int4_nominate.hip").read_text()
    assert "return (0.00390625f * 1.001f + (6.0f * d + 160.0f) * u) * (qn + norm_max) + 6.0f * u * (qn + mid[2 * dim_pad]) + 1e-30f;" in src
    header = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert "int32_t vg_index_enable_int4_nomination(vg_index *idx, int32_t on, void *stream);" in header
    assert "int32_t vg_index_int4_nomination_info(const vg_index *idx, int32_t *mode, int64_t *held_bytes, int64_t *rescanned);" in header


def worst_ratio(q, codes, mins, diff):
    """max over rows and two thresholds (a score of the set, flat_thr_cap_kernel's cap) of the error over eps"""
    dim = q.size
    ref = o.Int4Quantizer(dim)
    ref.set_params(mins, diff)
    c = np.stack([codes >> 4, codes & 15], axis=2).reshape(len(codes), -1).astype(np.float32)   # dimension 2 b: byte b's high nibble
    s = (diff / F(15.0)).astype(np.float32)
    mid = fma32(np.full(dim, 8.0, np.float32), s, mins)
    h2 = float(F(((np.abs(mins) + np.abs(diff)).astype(np.float64) ** 2).sum()))
    x = (((c / F(15.0)).astype(np.float32) * diff).astype(np.float32) + mins).astype(np.float32)
    y = ((c - F(8.0)) * s).astype(np.float32)
    nrm, cn = np.zeros(len(c), np.float32), np.zeros(len(c), np.float32)
    for j in range(dim):                # (the kernel's own order differs: the margin counts dim roundings, in any order)
        nrm, cn = fma32(x[:, j], x[:, j], nrm), fma32(y[:, j], y[:, j], cn)
    norm_max = float(max(nrm.max(), cn.max()))
    qn, shift = wave_sum(q, q), wave_sum(q, mid)
    eps = int4_eps(dim, float(qn), norm_max, h2)
    ex = np.array([ref.l2_distance(q, row) for row in codes], np.float64)
    bound = 2.002 * (float(qn) + norm_max)
    a, worst = rne_bf16((q * s).astype(np.float32)), 0.0
    for t in (F(min(max(float(np.median(ex)) - float(qn) + 2.0 * float(shift), -bound), bound)), F(bound)):
        acc = (F(0.5) * t - F(0.5) * nrm).astype(np.float32)
        for j in range(dim):            # K in element order, one rounding per accumulated product (bf16 x an integer: exact)
            acc = (acc + (a[j] * (c[:, j] - F(8.0))).astype(np.float32)).astype(np.float32)
        sc = (t - F(2.0) * acc).astype(np.float32)
        lhs = ((sc + qn).astype(np.float32) - F(2.0) * shift).astype(np.float32)
        assert np.isfinite(eps) and np.all(np.isfinite(sc))
        worst = max(worst, float(np.abs(lhs.astype(np.float64) - ex).max()) / eps)
    return worst


CASES = ["normal", "wide_dimension", "codes_0_or_15", "far_queries", "large_min", "all_8_huge_diff"]


@pytest.mark.parametrize("dim", [32, 96, 768])
@pytest.mark.parametrize("case", CASES)
def test_error_within_the_margin(case, dim):
    rng = np.random.default_rng(dim * 7 + CASES.index(case))
    rows = rng.standard_normal((96, dim)).astype(np.float32)
    if case == "wide_dimension":        # one dimension with a range 10^6 times the others
        rows[:, dim // 2] *= F(1e6)
    if case == "large_min":             # every row far from the origin: |min| >> diff
        rows += F(1000.0)
    q = (rows[3] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    iq = o.Int4Quantizer(dim)
    iq.train(rows)
    codes, mins, diff = iq.encode_batch(rows), iq.min.copy(), iq.diff.copy()
    if case == "codes_0_or_15":
        codes = np.where(rng.random(codes.shape) < 0.5, 0x00, 0xFF).astype(np.uint8)
        codes[0], codes[1] = 0x00, 0xFF                                       # an all-0 and an all-15 row
    if case == "far_queries":
        q = (1000.0 * rng.standard_normal(dim)).astype(np.float32)
    if case == "all_8_huge_diff":       # no row's norm bounds |min| + |diff|: every nibble of the even dimensions is 8
        diff[::2] *= F(1e4)
        mins[::2] = (-F(8.0) * diff[::2] / F(15.0) + F(0.3)).astype(np.float32)
        codes = ((codes & 0x0F) | 0x80).astype(np.uint8)
    worst = max(worst_ratio(qq, codes, mins, diff) for qq in (q, -q, (q * F(37.0)).astype(np.float32)))
    print(f"{case} dim={dim}: largest error / eps = {worst:.4f}")
    assert worst <= 1.0
