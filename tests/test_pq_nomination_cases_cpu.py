"""The builders of tests/pq_nomination_cases.py against the oracle alone: the near-tie rows really sit between the two
centroids they name, at the fractions of the kernels' margins they claim — so that tests/test_gpu_pq_nomination.py, which
only compares codes, cannot pass by testing nothing."""
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import pq_nomination_cases as pc

M = 4
BANDS = ((0, 0.5), (0.5, 1), (1, 2), (2, 16))


@functools.lru_cache(maxsize=None)
def case(mult, form):
    book = pc.offset_sweep(np.random.default_rng(5), M, mult)
    rows, pairs, t = pc.near_tie_rows(*book, form=form)
    cases = pairs.shape[1]
    opq = o.ProductQuantizer(M * pc.SD, M, pc.K)
    opq.set_codebooks(*book)
    return book, rows, pairs, t, cases, opq.encode_batch(rows[:cases])


def test_tile_constants_and_row_count():
    assert (pc.ROWS_PER_WAVE, pc.ROWS_PER_BLOCK) == (1024, 4096)
    _, rows, pairs, _, cases, _ = case(0, "bf16")
    # one case per (centroid, t, sign): exactly one workgroup tile, and a ragged second one behind it
    assert cases == pc.K * len(pc.TS) * 2 == pc.ROWS_PER_BLOCK
    assert rows.shape == (cases + pc.RAGGED, M * pc.SD) and np.array_equal(rows[cases:], rows[:pc.RAGGED])


def test_margins_are_the_kernels_formulae():
    """The float64 restatement at one hand-computed point: X = 4, C = 9 -> cross = 21, dmax = 25."""
    u, t16 = 2.0 ** -24, 2.0 ** -16
    bf16, fp32 = pc.margins(4.0, 9.0)
    assert fp32 == 1.05 * (64 * u * 21 + 24 * u * 25) + 1e-30
    assert bf16 == 1.05 * (2 * ((3.1 * t16 + 32 * u) * 21 + (1.01 * t16 + 32 * u) * 1.002 * 25) + 24 * u * 25) + 1e-30
    assert bf16 > 20 * fp32 > 0
    assert pc.margins(0.0, 0.0) == (1e-30, 1e-30)


@pytest.mark.parametrize("form", ["bf16", "fp32"])
@pytest.mark.parametrize("mult", [0, 1, 30])
def test_near_tie_rows_sit_where_they_claim(mult, form):
    book, rows, pairs, t, cases, codes = case(mult, form)
    v = pc.dequantise(*book).astype(np.float64)
    for s in range(M):
        x = rows[:cases, s * pc.SD:(s + 1) * pc.SD].astype(np.float64)
        a, b = pairs[s, :, 0], pairs[s, :, 1]
        # (a) in float64 the two nearest centroids are {a, b}, up to 1 % of the cases
        d = ((x[:, None, :] - v[s][None]) ** 2).sum(-1)
        two = np.sort(np.argsort(d, axis=1, kind="stable")[:, :2], axis=1)
        others = (two != np.sort(pairs[s], axis=1)).any(axis=1)
        assert others.mean() <= 0.01, (s, int(others.sum()))
        # (b) the oracle's code is a or b; it is the float64 winner wherever the row is at least 1 % of a margin off the bisector
        assert np.all((codes[:, s] == a) | (codes[:, s] == b)), s
        off = np.abs(t[s]) >= 0.01
        winner = np.where(t[s] > 0, a, b)
        assert np.array_equal(codes[off, s], winner[off]), s
        assert off.mean() >= 0.8
        # (c) every band of the achieved |t| is populated
        for lo, hi in BANDS:
            share = ((np.abs(t[s]) >= lo) & (np.abs(t[s]) < hi)).mean()
            assert share >= 0.05, (s, lo, hi, share)


def test_a_large_offset_lists_everything():
    """(d) At mult = 1000 the bf16 margin exceeds the squared distance of every centroid to its nearest neighbour: no pair can
    be accepted, the regime in which pq_fix_kernel decides everything.  (Nothing about {a, b} is claimed there.)"""
    book = pc.offset_sweep(np.random.default_rng(5), M, 1000)
    v = pc.dequantise(*book).astype(np.float64)
    for s in range(M):
        norms = (v[s] ** 2).sum(-1)
        _, spacing2 = pc.nearest_other(v[s])
        assert (pc.margins(norms, norms.max())[0] / spacing2).min() > 1.0, s


def test_offset_sweep_rows_stay_near_their_centroid():
    rng = np.random.default_rng(7)
    book = pc.offset_sweep(rng, M, 10)
    assert np.all(np.abs(book[2]) == np.float32(1.0)) and np.all((book[1] >= 0.005) & (book[1] < 0.025))
    x = pc.offset_sweep_rows(rng, *book, 500)
    v = pc.dequantise(*book).astype(np.float64)
    for s in range(M):
        d = ((x[:, None, s * pc.SD:(s + 1) * pc.SD].astype(np.float64) - v[s][None]) ** 2).sum(-1)
        spacing = np.sqrt(pc.nearest_other(v[s])[1]).mean()
        # noise of 0.3 spacing per coordinate: |noise| ~ 0.3 sqrt(8) spacing
        assert 0.4 * spacing < np.sqrt(d.min(axis=1)).mean() < 1.2 * spacing, s


def test_lattice_rows_tie():
    x = pc.lattice_rows(np.random.default_rng(74), 5157, 32)
    assert x.dtype == np.float32 and np.abs(np.rint(x)).max() == 2
    jitter = np.abs(x.astype(np.float64) - np.rint(x))
    steps = np.unique(jitter[jitter > 0])
    assert set(steps.tolist()) == {2.0 ** -10, 2.0 ** -14, 2.0 ** -18, 2.0 ** -22}
    # exact ties: squared distances between the lattice points themselves are small integers, shared by many pairs
    sub = np.rint(x[:300, :8])
    d = ((sub[:, None] - sub[None]) ** 2).sum(-1)
    assert np.unique(d).size < 100


def test_magnitude_rows_cover_every_special():
    x, where = pc.magnitude_rows(np.random.default_rng(41), pc.ROWS_PER_BLOCK + 70, M)
    n = x.shape[0]
    assert set(where) == {name for name, _ in pc.SPECIALS}
    with np.errstate(over="ignore", invalid="ignore"):
        X = (x[:, :8].astype(np.float32) ** 2).sum(-1, dtype=np.float32)
        assert np.all(X[where["denormal_square"]] == 0) and np.all(X[where["below_floor"]] < 1e-30)
        assert np.all((X[where["huge_nominated"]] > 1e29) & (X[where["huge_nominated"]] < 1e30))
        assert np.all((X[where["over_guard"]] >= 1e30) & np.isfinite(X[where["over_guard"]]))
        assert np.all(np.isinf((x[where["overflow"]].astype(np.float32) ** 2).sum(-1, dtype=np.float32)))
    assert np.all(np.signbit(x[where["minus_zero"]])) and np.all(x[where["zero"]] == 0)
    assert np.all(np.isnan(x[where["nan"]]).sum(axis=1) == 1) and (n - 1) in where["nan"]
    assert np.all(np.isposinf(x[where["plus_inf"]]).sum(axis=1) == 1)
    assert np.all(np.isneginf(x[where["minus_inf"]]).sum(axis=1) == 1)
    special = sorted(p for spots in where.values() for p in spots)
    assert len(special) == len(set(special)) and np.diff(special).min() >= 2   # finite rows in between
    assert {p % 32 for p in special} == set(range(32))                           # every lane position of a matrix tile
