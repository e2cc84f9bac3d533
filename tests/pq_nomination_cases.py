"""Inputs that put the decision seams of the PQ nominate-then-prove path (k_pq_train.hip: pq_nominate_bf16_kernel,
pq_nominate_kernel, pq_fix_kernel) under the data instead of leaving them to chance: rows a chosen fraction of the
kernels' own margin away from the bisector of two neighbouring centroids, codebooks whose offset makes the nominated
scores cancel, lattice rows with exact and near ties, and the row counts around a wave and a workgroup tile.

Plain numpy builders: tests/test_pq_nomination_cases_cpu.py checks them against the oracle alone,
tests/test_gpu_pq_nomination.py runs the library on them."""
import re
from pathlib import Path

import numpy as np

K = 256    # centroids per sub-quantizer and
SD = 8     # sub-dimension for which Encode / Train take the nomination (k_pq_train.hip:1451, :1540)

_SRC = (Path(__file__).resolve().parent.parent / "vecgo_amd" / "csrc" / "k_pq_train.hip").read_text()
# k_pq_train.hip:907: rows per wave and per workgroup of both nomination kernels
ROWS_PER_WAVE = int(re.search(r"kNomRowsPerWave = (\d+)", _SRC).group(1))
ROWS_PER_BLOCK = int(re.search(r"kNomRowsPerBlock = (\d+) \* kNomRowsPerWave", _SRC).group(1)) * ROWS_PER_WAVE

# the four forms of the path -> the hook that selects it (vg_internal.hpp:87-89)
FORMS = {"bf16": None, "fp32": "VG_PQ_FP32_MFMA", "list_all": "VG_PQ_LIST_ALL", "no_mfma": "VG_PQ_NO_MFMA"}

TS = (0, 0.01, 0.1, 0.5, 0.9, 1.1, 2, 8)
RAGGED = 37   # copies of early rows behind the one full tile of near_tie_rows


def margins(X, C):
    """(bf16 margin, fp32 margin) in float64 for |x_sub|^2 = X and C = max_c |v_c|^2: the gap between the two smallest
    scores above which a nomination kernel accepts its own answer.
    bf16: k_pq_train.hip:1294-1297 (derivation :1089-1093); fp32: k_pq_train.hip:1057-1059 (derivation :899-903)."""
    X = np.asarray(X, np.float64)
    C = np.asarray(C, np.float64)
    u, t16 = 2.0 ** -24, 2.0 ** -16
    sx, sc = np.sqrt(X), np.sqrt(C)
    cross = 2.0 * sx * sc + C
    dmax = (sx + sc) ** 2
    bf16 = 1.05 * (2.0 * ((3.1 * t16 + 32.0 * u) * cross + (1.01 * t16 + 32.0 * u) * 1.002 * dmax) + 24.0 * u * dmax) + 1e-30
    fp32 = 1.05 * (64.0 * u * cross + 24.0 * u * dmax) + 1e-30
    return bf16, fp32


def dequantise(codebooks, scales, offsets):
    """[m][256][8] float32 centroids as the library and the reference form them: two rounded float32 operations
    (pq.go:205-215)."""
    scales = np.asarray(scales, np.float32)
    offsets = np.asarray(offsets, np.float32)
    m = scales.size
    cb = np.asarray(codebooks, np.int8).reshape(m, K, SD).astype(np.float32)
    step = (cb * scales[:, None, None]).astype(np.float32)
    return (step + offsets[:, None, None]).astype(np.float32)


def nearest_other(v64):
    """For [256][8] float64 centroids: index of each centroid's nearest other centroid and the squared distance to it."""
    d = ((v64[:, None, :] - v64[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    b = d.argmin(1)
    return b, d[np.arange(v64.shape[0]), b]


def gaps(x_sub, v64, a, b):
    """float64 D_b - D_a of float32 sub-vectors x_sub [cases][8] against centroids a[i], b[i] of v64."""
    x = np.asarray(x_sub, np.float64)
    return ((x - v64[b]) ** 2).sum(-1) - ((x - v64[a]) ** 2).sum(-1)


def near_tie_rows(codebooks, scales, offsets, ts=TS, form="bf16"):
    """Rows whose sub-vector of every sub-quantizer sits t * margin (form's margin, `margins`) off the bisector of a centroid
    a and its nearest other centroid b: case (a, t, sign) is mid(a, b) -/+ e (v_b - v_a) with e = t margin / (2 |v_b - v_a|^2),
    rounded to float32, so that in float64 D_b - D_a = +/- t margin.  Row i carries case i of every sub-quantizer.
    Returns (rows [cases + RAGGED][8 m] float32, pairs [m][cases][2], achieved t [m][cases] (signed: > 0 = a is nearer),
    recomputed in float64 from the rounded row); the last RAGGED rows repeat the first ones."""
    assert form in ("bf16", "fp32")
    v = dequantise(codebooks, scales, offsets)
    m = v.shape[0]
    ts = np.asarray(ts, np.float64)
    cases = K * ts.size * 2
    a = np.repeat(np.arange(K), ts.size * 2)
    t = np.tile(np.repeat(ts, 2), K)
    sign = np.tile(np.array([1.0, -1.0]), K * ts.size)
    rows = np.empty((cases, m * SD), np.float32)
    pairs = np.empty((m, cases, 2), np.int64)
    achieved = np.empty((m, cases), np.float64)
    which = 0 if form == "bf16" else 1
    for s in range(m):
        v64 = v[s].astype(np.float64)
        nb, dist2 = nearest_other(v64)
        assert dist2.min() > 0.0, "two equal centroids: no bisector"
        C = (v64 ** 2).sum(-1).max()
        b = nb[a]
        mid = 0.5 * (v64[a] + v64[b])
        margin = margins((mid ** 2).sum(-1), C)[which]
        e = t * margin / (2.0 * dist2[a])
        x = (mid - (sign * e)[:, None] * (v64[b] - v64[a])).astype(np.float32)
        rows[:, s * SD:(s + 1) * SD] = x
        pairs[s, :, 0], pairs[s, :, 1] = a, b
        achieved[s] = gaps(x, v64, a, b) / margins((x.astype(np.float64) ** 2).sum(-1), C)[which]
    return np.concatenate([rows, rows[:RAGGED]]), pairs, achieved


def offset_sweep(rng, m, mult):
    """A random int8 codebook, scales in [0.005, 0.025), offsets +/- 0.1 mult: as mult grows C = max |v_c|^2 grows while the
    centroids' spacing stays, so the nominated scores cancel more and more and the margin has to list more and more pairs."""
    codebooks = rng.integers(-128, 128, m * K * SD).astype(np.int8)
    scales = (rng.random(m) * 0.02 + 0.005).astype(np.float32)
    offsets = (np.where(rng.random(m) < 0.5, -1.0, 1.0) * 0.1 * mult).astype(np.float32)
    return codebooks, scales, offsets


def offset_sweep_rows(rng, codebooks, scales, offsets, n):
    """n rows: in every sub-quantizer a centroid plus Gaussian noise of 0.3 x the mean nearest-centroid distance."""
    v = dequantise(codebooks, scales, offsets)
    m = v.shape[0]
    rows = np.empty((n, m * SD), np.float32)
    for s in range(m):
        spacing = np.sqrt(nearest_other(v[s].astype(np.float64))[1]).mean()
        c = rng.integers(0, K, n)
        rows[:, s * SD:(s + 1) * SD] = v[s][c] + (0.3 * spacing * rng.standard_normal((n, SD))).astype(np.float32)
    return rows


def lattice_rows(rng, n, dim):
    """Rows on the integer lattice {-2..2}^dim plus, per row, j 2^-k with j in {-1, 0, 1} per coordinate and k drawn from
    {10, 14, 18, 22}: against centroids that are data points (k-means++ seeds) the distances tie exactly or nearly."""
    base = rng.integers(-2, 3, (n, dim)).astype(np.float64)
    k = rng.choice(np.array([10, 14, 18, 22]), n)
    j = rng.integers(-1, 2, (n, dim)).astype(np.float64)
    rows = (base + j * (2.0 ** -k)[:, None]).astype(np.float32)
    assert np.array_equal(rows.astype(np.float64), base + j * (2.0 ** -k)[:, None])  # exact in float32
    return rows


def unit_vectors(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def few_distinct_rows(rng, n, m, few_subs, distinct=200):
    """Random rows in which the sub-vectors of the sub-quantizers `few_subs` take only `distinct` (< K) values, repeated:
    k-means++ runs into a zero running sum, Lloyd leaves clusters empty and converges at once."""
    rows = rng.standard_normal((n, m * SD)).astype(np.float32)
    for s in few_subs:
        pool = rng.standard_normal((distinct, SD)).astype(np.float32)
        rows[:, s * SD:(s + 1) * SD] = pool[np.arange(n) % distinct]
    return rows


# (name, value of every coordinate of the row's sub-vectors; None = see magnitude_rows)
SPECIALS = [("zero", 0.0), ("minus_zero", -0.0), ("denormal_square", 1e-40), ("below_floor", 1e-16),
            ("huge_nominated", 3e14), ("over_guard", 1e15), ("overflow", 1e19), ("nan", None), ("plus_inf", None),
            ("minus_inf", None)]


def magnitude_rows(rng, n, m):
    """n finite random rows with the SPECIALS put at positions that share a 32-row matrix tile with finite rows (every
    special row has finite neighbours) in the first and in the ragged second workgroup tile; the last rows, every second
    one, are one special of each kind, a NaN row the very last.  Returns (rows, {name: positions})."""
    dim = m * SD
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    where = {name: [] for name, _ in SPECIALS}

    def put(pos, name, value):
        if name == "nan":
            rows[pos, (pos * 5) % dim] = np.nan          # one NaN: one sub-quantizer's scores, the others stay finite
        elif name == "plus_inf":
            rows[pos, (pos * 3) % dim] = np.inf
        elif name == "minus_inf":
            rows[pos, (pos * 7) % dim] = -np.inf
        else:
            rows[pos] = np.float32(value)
        where[name].append(pos)

    # odd spacing: no two specials adjacent, every lane position of a 32-row tile is visited
    spots = list(range(3, n - 2 * len(SPECIALS), 67))
    for i, pos in enumerate(spots):
        put(pos, *SPECIALS[i % len(SPECIALS)])
    tail = [s for s in SPECIALS if s[0] != "nan"] + [("nan", None)]
    for i, spec in enumerate(tail):                      # the last rows, every second one: the very last row is special
        put(n - 1 - 2 * (len(tail) - 1 - i), *spec)
    return rows, where
