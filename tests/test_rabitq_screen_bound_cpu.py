"""The screen of the RaBitQ batch nomination (vg_index_enable_rabitq_nomination; vg_rabitq.hpp, rabitq_nom_gemm_kernel's epilogue),
without a GPU.

The GEMM has a pair's exact Hamming distance h and lists the row when the pair's exact score — rq.Distance in the reference's
operation order, one IEEE division per pair — MAY be at or below the query's threshold tau.  The screen multiplies instead:

    s~ = RN((qn - yn)^2 + RN(RN(RN(RN(4 qn) yn) * invd) * h)),   invd = RN(1 / dim) moved one ulp towards zero

and lists when s~ <= tau.  The proof of the nomination needs it CONSERVATIVE for stored norms that are not negative: whenever the
oracle's rabitq_distance <= tau, s~ <= tau — checked here over norms across the exponent range (subnormal products, the largest
finite, zero, Inf), h in {0, 1, dim / 2, dim}, dim in {1, 64, 768, 8192} and thresholds equal to the exact score and one ulp either
side.  The share of false passes (listed, exact score above tau) is printed: what the verify re-scores for nothing."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as o

ROOT = Path(__file__).resolve().parents[1]
F = np.float32


def invd(dim):
    """rq_screen_invd, restated"""
    r = F(1.0) / F(dim)
    return (np.array([r], F).view(np.uint32) - np.uint32(1)).view(F)[0]


def screen_score(qn, yn, h, dim):
    """the epilogue's s~, one float32 rounding per operation"""
    with np.errstate(all="ignore"):
        qn, yn, h = F(qn), F(yn), F(h)
        t1 = F(qn - yn)
        t1sq = F(t1 * t1)
        c = F(F(F(4.0) * qn) * yn)
        c = F(c * invd(dim))
        return F(t1sq + F(c * h))


def test_constants_are_the_librarys():
    src = (ROOT / "vecgo_amd" / "csrc" / "vg_rabitq.hpp").read_text()
    body = re.search(r"inline float rq_screen_invd\(int dim\)\s*\{(.*?)\n\}", src, flags=re.S).group(1)
    assert "1.0f / static_cast<float>(dim)" in body and "u -= 1;" in body
    gemm = (ROOT / "vecgo_amd" / "csrc" / "k_rabitq_nominate.hip").read_text()
    for line in ("const rn_f2 t1 = qn2 - y2;", "const rn_f2 t1sq = t1 * t1;", "rn_f2 c = a2 * y2;", "c = c * invd2;",
                 "const rn_f2 sc = t1sq + c * hf;", "const float a4 = 4.0f * qnv;"):
        assert line in gemm, line
    makefile = (ROOT / "vecgo_amd" / "csrc" / "Makefile").read_text()
    assert "-ffp-contract=off" in makefile          # c * hf and the sum stay two roundings


def pair(a, yn, h, dim):
    """a query (its norm set by one component a), a row code h bits away with stored norm yn; the oracle's distance and the
    query's norm as the oracle's Encode stores it"""
    nb = (dim + 63) // 64 * 8
    v = np.zeros(dim, F)
    v[0] = a
    with np.errstate(all="ignore"):
        qc = o.rabitq_encode(v)
    qn = qc[nb:].view(F)[0]
    code = qc.copy()
    b = np.unpackbits(code[:nb], bitorder="little")
    b[:h] ^= 1
    code[:nb] = np.packbits(b, bitorder="little")
    code[nb:] = np.frombuffer(F(yn).tobytes(), np.uint8)
    with np.errstate(all="ignore"):
        return qn, o.rabitq_distance(v, code)


TINY, HUGE = F(1e-45), np.finfo(F).max
QUERY_COMPONENTS = [0.0, 1e-22, 3e-20, 1e-10, 1e-3, 0.5, 1.0, 3.1415927, 1e3, 1e9, 1.7e19, 1.8446743e19, 1e20]     # the last: |q|^2 = Inf
STORED_NORMS = [0.0, TINY, 3e-45, 1e-40, 1.1754944e-38, 1e-30, 1e-20, 1e-7, 0.7, 1.0, 27.712812, 1e4, 1e15, 1e30, HUGE, np.inf]


def check(cases):
    """cases: (a, yn, h, dim).  Asserts the screen conservative on every case and threshold; returns (false passes, decisions)"""
    false_pass = decisions = 0
    for a, yn, h, dim in cases:
        qn, exact = pair(a, yn, h, dim)
        s = screen_score(qn, yn, h, dim)
        if np.isnan(exact):
            continue                                   # a NaN score is at or below nothing; the replay answers such queries
        with np.errstate(all="ignore"):
            taus = {exact, np.nextafter(exact, F(-np.inf)), np.nextafter(exact, F(np.inf))}
        for tau in taus:
            if np.isnan(tau):
                continue
            decisions += 1
            if exact <= tau:
                assert s <= tau, (a, qn, yn, h, dim, exact, s, tau)
            elif s <= tau:
                false_pass += 1
    return false_pass, decisions


@pytest.mark.parametrize("dim", [1, 64, 768, 8192])
def test_screen_is_conservative_on_adversarial_norms(dim):
    hs = sorted({0, 1, dim // 2, dim})
    cases = [(F(a), F(yn), h, dim) for a in QUERY_COMPONENTS for yn in STORED_NORMS for h in hs]
    fp, total = check(cases)
    print(f"dim {dim}: {len(cases)} pairs, {total} decisions, false passes {fp} ({fp / total:.3%})")
    assert total >= 3 * len(cases) // 2


@pytest.mark.parametrize("dim", [1, 64, 768, 8192])
def test_screen_is_conservative_on_random_norms(dim):
    """norms log-uniform over the whole exponent range, every h of a small dim, random h of a large one"""
    rng = np.random.default_rng(dim)
    m = 1500
    a = (2.0 ** rng.uniform(-74, 63, m)).astype(F)          # |q|^2 from subnormal to nearly the largest finite
    yn = (2.0 ** rng.uniform(-149, 127.9, m)).astype(F)
    yn[::7] = a[::7]                                          # equal norms: t1 = 0, the second term decides alone
    h = rng.integers(0, dim + 1, m)
    fp, total = check(zip(a, yn, h, [dim] * m))
    print(f"dim {dim}: {m} random pairs, {total} decisions, false passes {fp} ({fp / total:.3%})")


def test_a_negative_stored_norm_breaks_the_inequality():
    """why an index that holds one keeps the scan: the shrunk reciprocal makes the negative second term SMALLER in size"""
    qn, exact = pair(F(1.0), F(-1.0), 64, 64)
    assert screen_score(qn, F(-1.0), 64, 64) > exact
