"""The margin of the SQ8 nomination from the codes (vg_index_enable_sq8_nomination_from_codes; Sq8CodesRow::eps, k_sq8_scan.hip),
without a GPU.

The nomination GEMM multiplies the query image bf16(q_d * inv_d) — the only rounded operand — by the centred codes c - 128, which
bfloat16 holds exactly, with fp32 accumulation from the starting value (t - |x^|^2) / 2 (Dot: t) for the query's threshold t; its
score is s' = t - 2 acc (Dot: t - acc).  The proof compares the k-th exact score with tau + |q|^2 - 2 q.mid (Dot: -tau + q.mid),
mid_d = min_d + 128 inv_d, and holds only if |s' + |q|^2 - 2 q.mid - L2Distance| <= eps (Dot: |s' - q.mid + DotProduct| <= eps)
for every row, whatever the data.  This file models the operands in numpy — the same roundings, one fp32 rounding per accumulated
product, the norms, mid and q.mid in fp32 as the kernels compute them — and takes the exact score from the oracle's SQ8 distances
(sq8u_l2_batch, vgo_sq8_dot: the reference's own arithmetic)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as o

ROOT = Path(__file__).resolve().parent.parent
U = 2.0 ** -24
F = np.float32


def codes_eps(dot, dim, qn, norm_max, h2):
    """Sq8CodesRow::eps, restated"""
    if dot:
        return (2.0 ** -9 * 1.001 + (3.5 * dim + 64.0) * U) * (qn + norm_max) + U * (qn + h2) + 1e-30
    return (2.0 ** -8 * 1.001 + (6.0 * dim + 160.0) * U) * (qn + norm_max) + 1e-30


def test_formula_is_the_librarys():
    src = (ROOT / "vecgo_amd" / "csrc" / "k_sq8_scan.hip").read_text()
    body = re.search(r"struct Sq8CodesRow.*?__device__ float eps\(float qn, float norm_max\) const\s*\{(.*?)\n    \}", src, flags=re.S).group(1)
    assert "u = 5.9604645e-8f" in body
    assert "if (DOT) return (0.001953125f * 1.001f + (3.5f * d + 64.0f) * u) * (qn + norm_max) + u * (qn + mid[dim_pad]) + 1e-30f;" in body
    assert "return (0.00390625f * 1.001f + (6.0f * d + 160.0f) * u) * (qn + norm_max) + 1e-30f;" in body
    assert np.float32(5.9604645e-8) == np.float32(U) and 0.001953125 == 2.0 ** -9 and 0.00390625 == 2.0 ** -8


def rne_bf16(x):
    """bfloat16 round-to-nearest-even of finite float32 values, as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def fma32(a, b, c):
    """fp32 fused multiply-add of float32 arrays (a product of two float32 is exact in float64; the sum then rounds twice, which
    can differ from the fused result by one ulp in rare ties — far inside what the bound allows per operation)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def state(codes, mins, inv):
    """what the enable kernels keep: norms |x^|^2 (sequential fp32 fmas over the dimensions), norm_max = max(|x^|^2, |y|^2) over the
    rows, mid, H2"""
    n, dim = codes.shape
    cf = codes.astype(np.float32)
    x = fma32(cf, inv[None, :], mins[None, :])
    y = ((cf - F(128.0)) * inv[None, :]).astype(np.float32)
    nrm, cn = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for j in range(dim):
        nrm = fma32(x[:, j], x[:, j], nrm)
        cn = fma32(y[:, j], y[:, j], cn)
    mid = fma32(np.full(dim, 128.0, np.float32), inv, mins)
    h = (np.abs(mins) + F(255.0) * np.abs(inv)).astype(np.float32)
    h2 = F(0.0)
    for j in range(dim):
        h2 = F(np.float64(h[j]) * np.float64(h[j]) + np.float64(h2))
    return nrm, float(max(nrm.max(), cn.max())), mid, float(h2)


def model(q, codes, mins, inv, nrm, t, dot):
    """[n] GEMM scores s' of query q, threshold t: K in element order, one rounding per accumulated product"""
    a = rne_bf16((q * inv).astype(np.float32))
    cp = codes.astype(np.float32) - F(128.0)
    t = F(t)
    acc = np.full(len(codes), t, np.float32) if dot else (F(0.5) * t - F(0.5) * nrm).astype(np.float32)
    for j in range(q.size):
        acc = (acc + (a[j] * cp[:, j]).astype(np.float32)).astype(np.float32)   # bf16 x an integer below 2^8: exact in fp32
    return (t - acc).astype(np.float32) if dot else (t - F(2.0) * acc).astype(np.float32)


def wave_sum(q, w):
    """sum_j q_j w_j as a wave of 64 lanes computes it in fp32: lane l takes j = l, l + 64, ... by fma, then the xor tree"""
    part = np.zeros(64, np.float32)
    for j0 in range(0, q.size, 64):
        m = min(64, q.size - j0)
        part[:m] = fma32(q[j0:j0 + m], w[j0:j0 + m], part[:m])
    off = 32
    while off:
        part = (part + part[np.arange(64) ^ off]).astype(np.float32)
        off >>= 1
    return part[0]


def exact(q, codes, mins, inv, dot):
    if not dot:
        return o.sq8u_l2_batch(q, codes, mins, inv, q.size).astype(np.float64)
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    o.lib.vgo_sq8_dot.restype = C.c_float
    qq, mn, iv = (np.ascontiguousarray(v, np.float32) for v in (q, mins, inv))
    out = []
    for row in np.ascontiguousarray(codes, np.uint8):
        out.append(o.lib.vgo_sq8_dot(qq.ctypes.data_as(f32p), row.ctypes.data_as(u8p), C.c_int32(q.size), mn.ctypes.data_as(f32p),
                                     iv.ctypes.data_as(f32p)))
    return -np.asarray(out, np.float64)      # the search's Dot scores are -q.x^


def worst_ratio(q, codes, mins, inv, dot):
    """max over rows and thresholds of |s' + |q|^2 - 2 q.mid - exact| / eps (Dot: |s' - q.mid - exact|), every term but the exact
    score in fp32 as the verify kernels form it; the thresholds: a score of the set and flat_thr_cap_kernel's cap"""
    nrm, norm_max, mid, h2 = state(codes, mins, inv)
    qn = wave_sum(q, q)
    shift = wave_sum(q, mid)
    eps = codes_eps(dot, q.size, float(qn), norm_max, h2)
    assert np.isfinite(eps)
    ex = exact(q, codes, mins, inv, dot)
    bound = 2.002 * (float(qn) + norm_max)
    worst = 0.0
    for t in (None, bound):
        if t is None:
            t = float(np.median(ex)) - (0.0 if dot else float(qn)) + (1.0 if dot else 2.0) * float(shift)
            t = min(max(t, -bound), bound)
        s = model(q, codes, mins, inv, nrm, t, dot)
        assert np.all(np.isfinite(s))
        # the comparison's left side for a row sitting exactly at the threshold: (s' + qn) - 2 shift in fp32 (Dot: s' ... + shift)
        lhs = ((s + qn).astype(np.float32) - F(2.0) * shift).astype(np.float32) if not dot else (s - shift).astype(np.float32)
        worst = max(worst, float(np.abs(lhs.astype(np.float64) - ex).max()) / eps)
    return worst


def trained(rng, rows):
    """ScalarQuantizer.Train + Encode of the rows (the oracle's)"""
    sq = o.ScalarQuantizer(rows.shape[1])
    sq.train(rows)
    return sq.encode_batch(rows), sq.mins.copy(), sq.inv_scales.copy()


CASES = ["normal", "wide_dimension", "constant_dimensions", "codes_0_or_255", "far_queries", "all_128_huge_scale"]


def make(case, dim, rng):
    n = 96
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    q = (rows[3] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    if case == "wide_dimension":        # one dimension with a range 10^6 times the others
        rows[:, dim // 2] *= F(1e6)
        q = (rows[3] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    if case == "constant_dimensions":   # every row the same there: inv = 1e-6 / 255
        rows[:, ::2] = F(0.75)
        q = (rows[3] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    codes, mins, inv = trained(rng, rows)
    if case == "constant_dimensions":
        assert np.all(inv[::2] == F(F(1e-6) / F(255.0)) ) or np.all(inv[::2] < 1e-8)
    if case == "codes_0_or_255":
        codes = np.where(rng.random(codes.shape) < 0.5, 0, 255).astype(np.uint8)
        codes[0], codes[1] = 0, 255
    if case == "far_queries":           # queries 1000 x the rows
        q = (1000.0 * rng.standard_normal(dim)).astype(np.float32)
    if case == "all_128_huge_scale":    # no row's norm bounds |min| + 255 |inv|: every code of the even dimensions is 128
        inv[::2] *= F(1e4)
        mins[::2] = (-F(128.0) * inv[::2] + F(0.3)).astype(np.float32)
        codes[:, ::2] = 128
    return q, codes, mins, inv


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
@pytest.mark.parametrize("dim", [1, 17, 768])
@pytest.mark.parametrize("case", CASES)
def test_error_within_the_margin(case, dim, dot):
    rng = np.random.default_rng(dim * 7 + CASES.index(case))
    worst = 0.0
    for _ in range(2):
        q, codes, mins, inv = make(case, dim, rng)
        for qq in (q, -q, (q * F(37.0)).astype(np.float32)):
            worst = max(worst, worst_ratio(qq, codes, mins, inv, dot))
    print(f"{case} dim={dim} dot={dot}: largest error / eps = {worst:.4f}")
    assert worst <= 1.0


def test_uncentred_codes_would_need_a_wider_margin():
    """why the codes are centred: the same model with c in place of c - 128 (and min in place of mid) errs by more than this
    margin on normal rows — the query rounding is relative to |q| |x^ - min|"""
    rng = np.random.default_rng(3)
    dim = 768
    rows = rng.standard_normal((96, dim)).astype(np.float32)
    codes, mins, inv = trained(rng, rows)
    q = (rows[3] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    a = rne_bf16((q * inv).astype(np.float32)).astype(np.float64)
    qi = q.astype(np.float64) * inv.astype(np.float64)
    err_c = np.abs((a - qi) @ (codes.astype(np.float64) - 128.0).T).max()
    err_u = np.abs((a - qi) @ codes.astype(np.float64).T).max()
    print(f"query-rounding error of the dot product, centred {err_c:.4f}, uncentred {err_u:.4f}")
    assert err_u > 2.0 * err_c
