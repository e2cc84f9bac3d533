"""The margin of the flat search's screen (flat_gemm_screen_big_kernel, k_flat.hip screen_gemm_eps), without a GPU.

The screen scores a (query, row) pair as ONE bfloat16 product with fp32 accumulation: q.x ~ q_hi.x_hi, hi = bfloat16 round-to-
nearest-even, the accumulator starting at t (Dot) or (t - |x|^2) / 2 (L2) as in the split tile (tests/test_flat_split_bound.py,
whose helpers and conventions this file uses); the score is t - acc (Dot) or t - 2 acc (L2).  The screen's proof holds only if
that score is within screen_gemm_eps * (|q|^2 + max |x|^2) of the true one, whatever the data.

Tightness: the operand part of the bound is attained — every component 1 + 2^-8 is a tie that rounds to 1.0, both operands lose
2^-8 / (1 + 2^-8) of their value and all products err the same way; with query = row the modelled error / bound prints as 0.99
(dim 32) and 0.96 - 0.97 (dim 768, where the accumulation part is 2.3 % of the bound and sums of small integers round nowhere)."""
import re

import numpy as np
import pytest

from tests.test_flat_split_bound import ROOT, U16, U24, V, adversarial_corpus, rne_bf16, true_scores

U7, U8, U17 = 2.0 ** -7, 2.0 ** -8, 2.0 ** -17


def screen_eps(dot: bool, dim: int) -> float:
    """k_flat.hip screen_gemm_eps, restated"""
    m = (dim + 16) * U24
    return U8 + U17 + 2.52 * m if dot else U7 + U16 + 4.03 * m


def test_formula_is_the_librarys():
    src = (ROOT / "vecgo_amd" / "csrc" / "k_flat.hip").read_text()
    body = re.search(r"static float screen_gemm_eps\(bool dot, int dim\)\s*\{(.*?)\n\}", src, flags=re.S).group(1)
    assert "static_cast<float>(dim + 16) * 5.9604645e-8f" in body
    assert "dot ? 0.00390625f + 7.62939453125e-6f + 2.52f * m : 0.0078125f + 1.52587890625e-5f + 4.03f * m" in body
    assert (0.00390625, 7.62939453125e-6, 0.0078125, 1.52587890625e-5) == (U8, U17, U7, U16)
    assert np.float32(5.9604645e-8) == np.float32(U24)


def test_the_filters_factor_does_not_cover_the_accumulation():
    """why the margin is not the bfloat16 filter's 2^-7 * 1.02: at dim 768 that is below this tile's bound"""
    assert 0.0078125 * 1.02 < screen_eps(False, 768) and 0.00390625 * 1.02 < screen_eps(True, 768)
    assert 0.0078125 * 1.02 > screen_eps(False, 32)


def model_scores(q, rows, t, dot):
    """[len(rows)] scores of query q as the screen computes them, threshold t; float32 throughout, one rounding per product"""
    qh, xh = rne_bf16(q), rne_bf16(rows)
    norms = np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64)).astype(np.float32)
    t = np.float32(t)
    acc = np.full(len(rows), t, np.float32) if dot else (np.float32(0.5) * t - np.float32(0.5) * norms).astype(np.float32)
    for j in range(q.size):
        acc = (acc + (qh[j] * xh[:, j]).astype(np.float32)).astype(np.float32)       # a bf16 x bf16 product is exact in fp32
    sc = (t - acc).astype(np.float32) if dot else (t - np.float32(2.0) * acc).astype(np.float32)
    return sc, norms


def worst_ratio(q, rows, dot, thresholds=("score", "cap")):
    """max over rows and thresholds of |model - true| / (eps * (|q|^2 + max |x|^2)); the thresholds: a score of the set and
    flat_thr_cap_kernel's cap 2.002 (|q|^2 + max |x|^2)"""
    dim = q.size
    qn = float(q.astype(np.float64) @ q.astype(np.float64))
    norms64 = np.einsum("ij,ij->i", rows.astype(np.float64), rows.astype(np.float64))
    xmax = float(norms64.max())
    worst = 0.0
    for how in thresholds:
        t = 2.002 * (qn + xmax) if how == "cap" else float(np.median(true_scores(q, rows, norms64.astype(np.float32), dot)))
        sc, norms = model_scores(q, rows, t, dot)
        assert np.all(np.isfinite(sc))
        err = np.abs(sc.astype(np.float64) - true_scores(q, rows, norms, dot))
        worst = max(worst, float(err.max()) / (screen_eps(dot, dim) * (qn + xmax)))
    return worst


TIE = np.float32(1.0 + 2.0 ** -8)      # halfway between 1 and 1 + 2^-7: rounds to even, 1.0 — the largest relative loss of hi


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
@pytest.mark.parametrize("dim", [32, 768])
def test_worst_operand_pattern(dim, dot):
    """every component of query and rows at the rounding tie (and just under it: V), equal signs per product"""
    signs = np.where(np.arange(dim) % 3 == 0, -1.0, 1.0).astype(np.float32)
    for v in (TIE, V):
        q = np.full(dim, v, np.float32)
        rows = np.full((4, dim), v, np.float32)
        rows[1:, : dim // 2] = np.float32(1.0)        # rows that lose less: max |x|^2 is the first row's
        for qq, rr in ((q, rows), (q * signs, rows * signs), (q, -rows)):
            r = worst_ratio(qq, rr, dot)
            print(f"worst pattern dim={dim} dot={dot} v=1+{float(v) - 1.0:.3e}: error / bound = {r:.4f}")
            assert r <= 1.0
    rows, q, _ = adversarial_corpus(300, dim) if dim == 768 else (np.full((4, dim), V, np.float32), np.full(dim, V, np.float32), None)
    r = worst_ratio(q, rows, dot)
    print(f"adversarial corpus dim={dim} dot={dot}: error / bound = {r:.4f}")
    assert r <= 1.0


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
def test_heavy_cancellation(dot):
    """q.x ~ 0 at large |q||x|: the error is relative to the norms, not to the (tiny) dot product"""
    dim = 768
    rng = np.random.default_rng(11)
    q = (1000.0 * rng.standard_normal(dim)).astype(np.float32)
    r = 1000.0 * rng.standard_normal((128, dim))
    r -= np.outer(r @ q.astype(np.float64), q.astype(np.float64)) / float(q.astype(np.float64) @ q.astype(np.float64))
    ratio = worst_ratio(q, r.astype(np.float32), dot)
    print(f"cancellation dot={dot}: error / bound = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("dot", [False, True], ids=["L2", "Dot"])
def test_bound_is_not_simply_huge(dot):
    """the bound within 1.1x of the worst error constructed, at both dims (the operand part is attained)"""
    for dim in (32, 768):
        q = np.full(dim, TIE, np.float32)
        tight = 1.0 / worst_ratio(q, q[None, :].copy(), dot, thresholds=("score",))
        print(f"tightness dot={dot} dim={dim}: bound / worst constructed error = {tight:.3f}")
        assert 1.0 <= tight <= 1.1
