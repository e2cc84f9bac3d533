"""The margin of the flat search's split nomination tile (flat_gemm_split_big_kernel, k_flat.hip split_gemm_eps), without a GPU.

The tile scores a (query, row) pair as three bfloat16 products with fp32 accumulation: x = hi + lo (hi = bfloat16 round-to-
nearest-even of x, lo = the same of x - hi), q.x ~ q_hi.x_hi + q_lo.x_hi + q_hi.x_lo, the accumulator starting at t (Dot) or
(t - |x|^2) / 2 (L2) for the query's threshold t; the score is t - acc (Dot) or t - 2 acc (L2).  The proof of the search holds only
if that score is within eps_extra * (|q|^2 + max |x|^2) of the true one, whatever the data: this file models the arithmetic in
numpy (the same roundings, one fp32 rounding per accumulated product — the matrix unit rounds no more often than that) and
compares with float64.  "True" is |x|^2_stored - 2 q.x (L2, the row norm as the library stores it, fp32) or -q.x (Dot).

Tightness: the bound is a sum of a part for the dropped terms (3 * 2^-16 |q||x|) and a part for 3 dim + 16 roundings of the
accumulator, each worst case and linear in dim.  The worst error constructed here (every component just under the rounding
boundary of hi AND of lo, query = row, dim 32) reaches 1 / 2.4 (L2) and 1 / 2.7 (Dot) of it — inside the factor 4.  At dim 768
the accumulation part dominates (0.92 of the bound) and no input makes 2320 fp32 roundings all fall the same way: the same
construction reaches 1 / 62 (L2) and 1 / 76 (Dot) there, printed by test_bound_is_not_simply_huge, not asserted."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U16, U24 = 2.0 ** -16, 2.0 ** -24


def split_eps(dot: bool, dim: int) -> float:
    """k_flat.hip split_gemm_eps, restated"""
    m = (3 * dim + 16) * U24
    return 1.5001 * U16 + 2.52 * m if dot else 3.0002 * U16 + 4.03 * m


def test_formula_is_the_librarys():
    src = (ROOT / "vecgo_amd" / "csrc" / "k_flat.hip").read_text()
    body = re.search(r"static float split_gemm_eps\(bool dot, int dim\)\s*\{(.*?)\n\}", src, flags=re.S).group(1)
    assert "static_cast<float>(3 * dim + 16) * 5.9604645e-8f" in body
    assert "dot ? 1.5001f * 1.52587890625e-5f + 2.52f * m : 3.0002f * 1.52587890625e-5f + 4.03f * m" in body
    assert np.float32(5.9604645e-8) == np.float32(U24) and 1.52587890625e-5 == U16


def rne_bf16(x):
    """bfloat16 round-to-nearest-even of finite float32 values, as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def split(x):
    hi = rne_bf16(x)
    with np.errstate(invalid="ignore"):
        lo = rne_bf16((x - hi).astype(np.float32))
    return hi, lo


def model_scores(q, rows, t, dot):
    """[len(rows)] scores of query q as the tile computes them, threshold t; float32 throughout.  Order: K in groups of 16,
    per group q_hi.x_hi, q_lo.x_hi, q_hi.x_lo, one rounding per product."""
    qh, ql = split(q)
    xh, xl = split(rows)
    norms = np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64)).astype(np.float32)
    t = np.float32(t)
    acc = np.full(len(rows), t, np.float32) if dot else (np.float32(0.5) * t - np.float32(0.5) * norms).astype(np.float32)
    for g in range(0, q.size, 16):
        for a, b in ((qh, xh), (ql, xh), (qh, xl)):
            for j in range(g, g + 16):
                acc = (acc + (a[j] * b[:, j]).astype(np.float32)).astype(np.float32)   # a bf16 x bf16 product is exact in fp32
    sc = (t - acc).astype(np.float32) if dot else (t - np.float32(2.0) * acc).astype(np.float32)
    return sc, norms


def true_scores(q, rows, norms, dot):
    d = rows.astype(np.float64) @ q.astype(np.float64)
    return -d if dot else norms.astype(np.float64) - 2.0 * d


def worst_ratio(q, rows, dot, thresholds=("score", "cap")):
    """max over rows and thresholds of |model - true| / (eps * (|q|^2 + max |x|^2)); the thresholds: a score of the set (what a
    sample gives) and flat_thr_cap_kernel's cap 2.002 (|q|^2 + max |x|^2) (no sample)"""
    dim = q.size
    qn = float(q.astype(np.float64) @ q.astype(np.float64))
    norms64 = np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64))
    xmax = float(norms64.max())
    worst = 0.0
    for how in thresholds:
        if how == "cap":
            t = 2.002 * (qn + xmax)
        else:
            t = float(np.median(true_scores(q, rows, norms64.astype(np.float32), dot)))
        sc, norms = model_scores(q, rows, t, dot)
        assert np.all(np.isfinite(sc))
        err = np.abs(sc.astype(np.float64) - true_scores(q, rows, norms, dot))
        worst = max(worst, float(err.max()) / (split_eps(dot, dim) * (qn + xmax)))
    return worst


# v: just under the boundary of hi (1 + 2^-8 rounds to even = 1) and, for the remainder 2^-8 - 2^-17 - 2^-23, just under that of lo
# (2^-8 - 2^-16 | 2^-8): hi = 1, lo = 2^-8 - 2^-16, left over 2^-17 - 2^-23 — the dropped terms all have one sign
V = np.float32(1.0 + 2.0 ** -8 - 2.0 ** -17 - 2.0 ** -23)


def adversarial_corpus(n=4200, dim=768, seed=5):
    """rows [n, dim], query [dim], the ids of the three true nearest rows (L2), in order.  As test_filter_worst_case_rounding
    (tests/test_gpu_flat_bf16.py): the query and the three near rows are all V (j = 3, 4, 5 components one larger: distance j),
    every other row is 1.0 with 6 or 7 components 2.0 (distance 6.0x, 7.0x): the split loses the most on the near rows."""
    rng = np.random.default_rng(seed)
    rows = np.ones((n, dim), np.float32)
    for r in range(n):
        rows[r, rng.choice(dim, 6 if r % 273 == 1 else 7, replace=False)] = np.float32(2.0)
    near = []
    for j, rid in ((3, n // 2), (4, 17), (5, n - 100)):
        row = np.full(dim, V, np.float32)
        row[rng.choice(dim, j, replace=False)] += np.float32(1.0)
        rows[rid] = row
        near.append(rid)
    return rows, np.full(dim, V, np.float32), near


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
@pytest.mark.parametrize("dim", [32, 96, 768])
def test_random_vectors(dim, dot):
    rng = np.random.default_rng(dim)
    for scale in (1.0, 37.0):
        rows = (scale * rng.standard_normal((256, dim))).astype(np.float32)
        q = rng.standard_normal(dim).astype(np.float32)
        r = worst_ratio(q, rows, dot)
        print(f"random dim={dim} dot={dot} scale={scale}: error / bound = {r:.4f}")
        assert r <= 1.0


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
@pytest.mark.parametrize("dim", [32, 768])
def test_components_just_under_a_rounding_boundary(dim, dot):
    rows, q, near = adversarial_corpus(300, dim) if dim == 768 else (np.full((4, dim), V, np.float32), np.full(dim, V, np.float32), None)
    signs = np.where(np.arange(dim) % 3 == 0, -1.0, 1.0).astype(np.float32)     # and with mixed signs, the same boundary
    for qq, rr in ((q, rows), (q * signs, rows * signs), (q, -rows)):
        r = worst_ratio(qq, rr, dot)
        print(f"boundary dim={dim} dot={dot}: error / bound = {r:.4f}")
        assert r <= 1.0


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
def test_heavy_cancellation(dot):
    """q.x ~ 0 at large |q||x|: the error is relative to the norms, not to the (tiny) dot product"""
    dim = 768
    rng = np.random.default_rng(11)
    q = (1000.0 * rng.standard_normal(dim)).astype(np.float32)
    r = 1000.0 * rng.standard_normal((128, dim))
    r -= np.outer(r @ q.astype(np.float64), q.astype(np.float64)) / float(q.astype(np.float64) @ q.astype(np.float64))
    rows = r.astype(np.float32)
    d = rows.astype(np.float64) @ q.astype(np.float64)
    assert np.abs(d).max() < 1e-4 * 1e6 * dim        # |q||x| ~ 7.7e8 per row, the dot products ~ 1e1
    ratio = worst_ratio(q, rows, dot)
    print(f"cancellation dot={dot}: error / bound = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
def test_mixed_magnitudes(dot):
    """components from 1e-20 to 1e18 in one vector (squares up to 1e36: the norms stay finite)"""
    dim = 768
    rng = np.random.default_rng(13)
    def mixed(shape):
        return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-20, 18, shape)).astype(np.float32)
    rows, q = mixed((128, dim)), mixed(dim)
    ratio = worst_ratio(q, rows, dot)
    print(f"mixed magnitudes dot={dot}: error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    small = (rows * np.float32(1e-19)).astype(np.float32)        # down to 1e-39: denormal components
    with np.errstate(under="ignore"):
        ratio = worst_ratio((q * np.float32(1e-19)).astype(np.float32), small, dot, thresholds=("score",))
    assert ratio <= 1.0


def test_the_near_rows_of_the_adversarial_corpus_are_the_hardest():
    rows, q, near = adversarial_corpus(600)
    sc, norms = model_scores(q, rows, 20.0, False)
    err = sc.astype(np.float64) - true_scores(q, rows, norms, False)
    order = np.argsort(true_scores(q, rows, norms, False), kind="stable")
    assert order[:3].tolist() == near
    assert np.abs(err[near]).min() > 4 * np.abs(np.delete(err, near)).max()      # the split is exact on 1.0 / 2.0


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
def test_bound_is_not_simply_huge(dot):
    """the bound within 4x of the worst error constructed (dim 32, query = row = all V); the ratio at dim 768 is printed"""
    out = {}
    for dim in (32, 768):
        q = np.full(dim, V, np.float32)
        out[dim] = 1.0 / worst_ratio(q, q[None, :].copy(), dot, thresholds=("score",))
        print(f"tightness dot={dot} dim={dim}: bound / worst constructed error = {out[dim]:.2f}")
    assert out[32] <= 4.0
