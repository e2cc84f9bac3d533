"""ProductQuantizer Encode and the Lloyd assignment of Train at the decision seams of the nominate-then-prove path
(k_pq_train.hip: pq_nominate_bf16_kernel / pq_nominate_kernel accept a centroid when the two smallest scores are further
apart than a margin, pq_fix_kernel decides the rest): rows placed a fraction of that margin off a bisector, codebooks that
make the scores cancel, magnitudes around the margin's floor and guard, non-finite rows beside finite ones, the row
counts around a wave, a workgroup tile and a row chunk.  Every expected value is the oracle's, every comparison exact;
each of the four forms (tests/pq_nomination_cases.py: FORMS) is compared with the oracle, never with another form."""
import functools

import numpy as np
import pytest

from oracle import oracle as o
from tests import pq_nomination_cases as pc
from tests.hooks import set_hook

pytestmark = pytest.mark.gpu

WAVE, BLOCK = pc.ROWS_PER_WAVE, pc.ROWS_PER_BLOCK
ALL_FORMS = list(pc.FORMS)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def in_form(form, fn):
    hook = pc.FORMS[form]
    if hook:
        set_hook(hook, 1)
    try:
        return fn()
    finally:
        if hook:
            set_hook(hook, 0)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def oracle_pq(m, book):
    opq = o.ProductQuantizer(m * pc.SD, m, pc.K)
    opq.set_codebooks(*book)
    return opq


def assert_encode(vg, ctx, form, m, book, x, want, what):
    pq = vg.ProductQuantizer(ctx, m * pc.SD, m, pc.K)
    pq.set_codebooks(*book)
    got = in_form(form, lambda: pq.encode(x))
    diff = np.argwhere(got != want)
    assert diff.shape[0] == 0, (what, form, f"{diff.shape[0]} of {want.size} codes differ; first (row, sub-quantizer): "
                                f"{diff[:5].tolist()}, got {got[tuple(diff[0])]} want {want[tuple(diff[0])]}")


def assert_train(vg, ctx, form, m, x, iters, seed, want, what):
    pq = vg.ProductQuantizer(ctx, m * pc.SD, m, pc.K)
    in_form(form, lambda: pq.train(x, iters=iters, seed=seed))
    cb, sc, of = pq.codebooks()
    wcb, wsc, wof = want
    assert np.array_equal(cb, wcb), (what, form, f"{int((cb != wcb).sum())} codebook bytes differ, sub-quantizers "
                                     f"{sorted(set((np.flatnonzero(cb != wcb) // (pc.K * pc.SD)).tolist()))}")
    assert np.array_equal(bits(sc), bits(wsc)), (what, form, "scales")
    assert np.array_equal(bits(of), bits(wof)), (what, form, "offsets")


@functools.lru_cache(maxsize=None)
def oracle_train(key, m, iters, seed):
    x = TRAIN_ROWS[key]()
    opq = o.ProductQuantizer(m * pc.SD, m, pc.K)
    opq.train(x, iters=iters, seed=seed)
    return frozen(x, opq.codebooks.copy(), opq.scales.copy(), opq.offsets.copy())


# ---- Encode ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def near_tie_case(m, mult, margin_form):
    book = pc.offset_sweep(np.random.default_rng(5), m, mult)
    x, _, _ = pc.near_tie_rows(*book, form=margin_form)
    return frozen(*book, x, oracle_pq(m, book).encode_batch(x))


@pytest.mark.parametrize("form", ALL_FORMS)
@pytest.mark.parametrize("mult", [0, 1, 30])
@pytest.mark.parametrize("m", [4, 32])     # pq_nom_block: the plain and the XCD-interleaved workgroup order
def test_encode_near_ties(vg, ctx, m, mult, form):
    """One full tile of rows 0 .. 8 margins either side of a bisector (placed with the margin of the form under test), and
    a ragged second tile."""
    *book, x, want = near_tie_case(m, mult, "fp32" if form == "fp32" else "bf16")
    assert x.shape[0] == BLOCK + pc.RAGGED
    assert_encode(vg, ctx, form, m, book, x, want, ("near ties", m, mult))


SWEEP_N = BLOCK + WAVE + 37


@functools.lru_cache(maxsize=None)
def sweep_case(mult):
    rng = np.random.default_rng(11 + mult)
    book = pc.offset_sweep(rng, 4, mult)
    x = pc.offset_sweep_rows(rng, *book, SWEEP_N)
    return frozen(*book, x, oracle_pq(4, book).encode_batch(x))


@pytest.mark.parametrize("form", ALL_FORMS)
@pytest.mark.parametrize("mult", [0, 10, 100, 1000, 10 ** 4])
def test_encode_offset_sweep(vg, ctx, mult, form):
    *book, x, want = sweep_case(mult)
    assert_encode(vg, ctx, form, 4, book, x, want, ("offset sweep", mult))


SEAM_NS = [1, 31, 33, WAVE - 1, WAVE + 1, BLOCK - 1, BLOCK + 1, BLOCK + WAVE + 1]


@functools.lru_cache(maxsize=None)
def row_seam_case(m):
    """The longest call's rows and the oracle's codes; a shorter call takes the first n of both."""
    rng = np.random.default_rng(300 + m)
    book = (rng.integers(-128, 128, m * pc.K * pc.SD).astype(np.int8), (rng.random(m) * 0.02 + 0.005).astype(np.float32),
            ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32))
    x = rng.standard_normal((max(SEAM_NS), m * pc.SD)).astype(np.float32)
    return frozen(*book, x, oracle_pq(m, book).encode_batch(x))


@pytest.mark.parametrize("form", ["bf16", "fp32"])
@pytest.mark.parametrize("m", [1, 3, 32, 96])
@pytest.mark.parametrize("n", SEAM_NS)
def test_encode_row_seams(vg, ctx, n, m, form):
    """One row, one short of / one past a 32-row matrix tile, a wave's rows and a workgroup's rows; a ragged wave in a
    second workgroup tile."""
    *book, x, want = row_seam_case(m)
    assert_encode(vg, ctx, form, m, book, np.ascontiguousarray(x[:n]), want[:n], ("row seams", n, m))


@functools.lru_cache(maxsize=None)
def magnitude_case():
    rng = np.random.default_rng(41)
    book = pc.offset_sweep(rng, 4, 1)
    x, where = pc.magnitude_rows(rng, BLOCK + 70, 4)
    return frozen(*book, x, oracle_pq(4, book).encode_batch(x)) + (where,)


@pytest.mark.parametrize("form", ALL_FORMS)
def test_encode_magnitudes_and_non_finite_rows(vg, ctx, form):
    """Zero, denormal-square, below the margin's 1e-30 floor, just under and over the X + C < 1e30 guard, overflowing,
    NaN and +/-Inf rows, each between finite rows of its 32-row matrix tile, and as the very last row of a ragged wave."""
    *book, x, want, where = magnitude_case()
    n = x.shape[0]
    assert n == BLOCK + 70 and not np.isfinite(x[n - 1]).all()
    for name, spots in where.items():
        assert len(spots) >= 2 and min(spots) < BLOCK - 32 and max(spots) >= BLOCK, name
        for p in spots:   # a finite row shares the 32-row tile
            assert any(np.isfinite(x[q]).all() and np.abs(x[q]).max() < 10 for q in (p - 1, p + 1) if q // 32 == p // 32 and q < n), name
    assert_encode(vg, ctx, form, 4, book, x, want, "magnitudes")


@functools.lru_cache(maxsize=None)
def inf_scale_case():
    rng = np.random.default_rng(43)
    cb, sc, of = pc.offset_sweep(rng, 4, 1)
    sc[2] = np.inf        # C of sub-quantizer 2 is not finite: all of its pairs are listed
    x = rng.standard_normal((WAVE + 37, 32)).astype(np.float32)
    return frozen(cb, sc, of, x, oracle_pq(4, (cb, sc, of)).encode_batch(x))


@pytest.mark.parametrize("form", ALL_FORMS)
def test_encode_with_a_non_finite_scale(vg, ctx, form):
    *book, x, want = inf_scale_case()
    assert_encode(vg, ctx, form, 4, book, x, want, "scale +Inf in sub-quantizer 2")


def test_encode_across_row_chunks(vg, ctx):
    """vg_pq_encode walks the rows in chunks of floor((2^28 / 8 m) / 4096) * 4096 (k_pq_train.hip:1543-1544: 348 160 rows at
    m = 96); row_first > 0 needs n m > 2^25 pairs whatever m is, so this is the smallest call with a second chunk: one
    more workgroup tile and a ragged wave behind the first chunk.  The rows are made on the device."""
    import torch
    m, dim = 96, 96 * pc.SD
    chunk = ((1 << 28) // (8 * m)) // BLOCK * BLOCK
    n = chunk + BLOCK + 37
    rng = np.random.default_rng(96)
    book = (rng.integers(-128, 128, m * pc.K * pc.SD).astype(np.int8), (rng.random(m) * 0.02 + 0.005).astype(np.float32),
            ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32))
    pq = vg.ProductQuantizer(ctx, dim, m, pc.K)
    pq.set_codebooks(*book)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(96)
    x = torch.randn((n, dim), device="cuda", dtype=torch.float32, generator=gen)
    torch.cuda.synchronize()
    whole = pq.encode(x)
    assert isinstance(whole, torch.Tensor) and tuple(whole.shape) == (n, m)
    # (i) the rows from one tile before the chunk's end on, encoded on their own (row_first = 0 throughout)
    first = chunk - BLOCK
    alone = pq.encode(x[first:])
    torch.cuda.synchronize()
    assert torch.equal(whole[first:], alone)
    # (ii) the oracle on the rows either side of the chunk's end and on the last rows
    opq = oracle_pq(m, book)
    for lo, hi in ((chunk - 64, chunk + 64), (n - 101, n)):
        got = whole[lo:hi].cpu().numpy()
        want = opq.encode_batch(x[lo:hi].cpu().numpy())
        assert np.array_equal(got, want), (lo, hi, int((got != want).sum()))
    del x, whole, alone
    torch.cuda.empty_cache()   # 1.1 GB of rows: not left in the caching allocator for the rest of the suite


# ---- Train -----------------------------------------------------------------------------------------------------------------

TRAIN_ROWS = {
    ("unit", BLOCK + WAVE + 37, 32): lambda: pc.unit_vectors(np.random.default_rng(71), BLOCK + WAVE + 37, 32 * pc.SD),
    ("unit", BLOCK + 1, 4): lambda: pc.unit_vectors(np.random.default_rng(72), BLOCK + 1, 4 * pc.SD),
    ("unit", WAVE - 1, 1): lambda: pc.unit_vectors(np.random.default_rng(73), WAVE - 1, pc.SD),
    ("lattice", BLOCK + WAVE + 37, 4): lambda: pc.lattice_rows(np.random.default_rng(74), BLOCK + WAVE + 37, 4 * pc.SD),
    ("few", BLOCK + 33, 4): lambda: pc.few_distinct_rows(np.random.default_rng(75), BLOCK + 33, 4, (0, 2)),
}


@pytest.mark.parametrize("form", ALL_FORMS)
@pytest.mark.parametrize("n,m,iters", [(BLOCK + WAVE + 37, 32, 3), (BLOCK + 1, 4, 3), (WAVE - 1, 1, 2)])
def test_train_seams(vg, ctx, n, m, iters, form):
    """Two workgroup tiles with a ragged wave in the XCD-interleaved order; one row past a tile; one row short of a wave."""
    x, *want = oracle_train(("unit", n, m), m, iters, 42)
    assert_train(vg, ctx, form, m, x, iters, 42, want, ("train seams", n, m))


@pytest.mark.parametrize("form", ALL_FORMS)
def test_train_near_ties(vg, ctx, form):
    """Lattice rows: exact and near ties against the k-means++ seeds (data points) and their means.  n / k is about 20 on
    purpose: one wrongly assigned point moves a centroid by about 1/20 of a cluster radius, several int8 steps of the
    codebook, the only output Train has."""
    n, m = BLOCK + WAVE + 37, 4
    x, *want = oracle_train(("lattice", n, m), m, 2, 42)
    assert_train(vg, ctx, form, m, x, 2, 42, want, "train near ties")


@pytest.mark.parametrize("form", ALL_FORMS)
def test_train_sub_quantizers_finish_at_different_iterations(vg, ctx, form):
    """Sub-quantizers 0 and 2 hold 200 distinct sub-vectors (< k: zero running sum in k-means++, empty clusters, Lloyd
    converges at once and done[sub] is set early) while 1 and 3 go on: the nomination's per-sub-quantizer early exit."""
    n, m = BLOCK + 33, 4
    x, *want = oracle_train(("few", n, m), m, 8, 42)
    assert_train(vg, ctx, form, m, x, 8, 42, want, "train done[] early exit")
