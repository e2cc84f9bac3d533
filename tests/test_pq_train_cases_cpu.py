"""tests/pq_train_cases.py against the oracle alone: the conditions under which tests/test_gpu_pq_train_seams.py cannot pass
vacuously — the row counts sit on the seams they name, the k-means++ picks of the large cases really come from behind
the first scan chunk, the fallback cases really end in the walk's fallback, and the degenerate cases really are."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import pq_train_cases as pc


def seeds_of(case):
    """(float32 seeds [m, k, sd], decoded int8 seeds [m, k, sd], int8 codebook [m, k, sd], scales) at iters = 0."""
    if case.name not in _SEEDS:
        _SEEDS[case.name] = _seeds_of(case)
    return _SEEDS[case.name]


_SEEDS = {}


def _seeds_of(case):
    opq = o.ProductQuantizer(case.dim, case.m, case.k)
    opq.train(case.rows(), iters=0, seed=case.seed)
    shape = (case.m, case.k, case.sd)
    return (opq.centroids_f32.reshape(shape).copy(), pc.decode(opq.codebooks, opq.scales, opq.offsets, *shape),
            opq.codebooks.reshape(shape).copy(), opq.scales.copy())


def sub_rows(case, sub):
    return case.rows()[:, sub * case.sd:(sub + 1) * case.sd]


def assert_seeds_are_rows(case):
    """Without a Lloyd iteration every centroid is a training sub-vector, bit for bit."""
    f32 = seeds_of(case)[0]
    for sub in range(case.m):
        have = {r.tobytes() for r in np.ascontiguousarray(sub_rows(case, sub))}
        assert all(c.tobytes() in have for c in f32[sub]), (case.name, sub)


def test_constants_are_the_kernels():
    assert (pc.PP_THREADS, pc.PP_BLOCK, pc.PP_SCAN, pc.ASSIGN_ROWS) == (1024, 64, 4096, 4)
    assert pc.UNROLL_RULE in pc._SRC and "kTrip = (kPPThreads / 64) * kPPUnroll;" in pc._SRC
    assert "in_lds = nblk <= kPPScan;" in pc._SRC
    assert {sd: pc.trip_rows(sd) for sd in (4, 8, 16)} == {4: 4096, 8: 3072, 16: 2048}
    assert pc.LDS_ROWS == 262_144


def test_case_names_and_shapes():
    cases = list(pc.all_cases()) + [pc.a4_case()]
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    for c in cases:
        x = c.rows()
        assert x.shape == (c.n, c.dim) and x.dtype == np.float32 and not x.flags.writeable, c.name
        assert np.isfinite(x).all(), c.name
    assert pc.a3_case().n == 2 * 262_144 + 64 * 17 + 5
    assert {c.name for c in pc.c_cases()} == {name for name, _, _ in pc.C_SHAPES}


def test_numpy_rng_is_the_oracles():
    seeds = [1, 2, 156712, 2 ** 40 + 5, 2 ** 64 - 1]
    for a, b, c in ((0, 1, 0), (0, 1, 1), (3, 2, 7)):
        with np.errstate(over="ignore"):
            got = pc.rng_u64_np(np.array(seeds, np.uint64), a, b, c)
        assert [int(v) for v in got] == [o.rng_u64(s, a, b, c) for s in seeds]


# ---- A ---------------------------------------------------------------------------------------------------------------------
def test_a1_sits_on_the_lds_boundary():
    inside, outside = pc.a1_cases()
    assert pc.nblk(inside.n) == pc.PP_SCAN and pc.nblk(outside.n) == pc.PP_SCAN + 1
    assert outside.n % pc.PP_BLOCK == 1          # the second scan chunk is one block that holds one row
    assert (inside.m, inside.sd, inside.k, inside.iters) == (2, 8, 8, (0, 1))
    assert np.array_equal(inside.rows(), outside.rows()[:inside.n])
    assert_seeds_are_rows(outside)


@pytest.mark.parametrize("case", list(pc.a2_cases()), ids=lambda c: c.name)
def test_a2_seeds_come_from_both_sides_of_the_first_chunk(case):
    assert pc.nblk(case.n) == pc.PP_SCAN + 17 and case.n % pc.PP_BLOCK == 1 and case.m == 2
    x = case.rows()
    for sub in range(case.m):
        marker = x[:, sub * case.sd]
        assert (marker[:pc.A2_HEAD] <= -0.5).all() and (marker[pc.A2_HEAD:] >= 0.5).all()
    f32, dec, cb, _ = seeds_of(case)
    assert_seeds_are_rows(case)
    splits = []
    for sub in range(case.m):
        tail = dec[sub, :, 0] > 0
        assert np.array_equal(tail, f32[sub, :, 0] > 0), (case.name, sub)   # int8 keeps the marker's sign
        splits.append((int((~tail).sum()), int(tail.sum())))
        assert 1 <= tail.sum() <= case.k - 1, (case.name, sub, splits)      # tail: rows of blocks >= 4096
        assert np.unique(cb[sub], axis=0).shape[0] == case.k, (case.name, sub)
    print(case.name, "head/tail seeds per sub-quantizer:", splits)


def test_a3_seeds_come_from_behind_the_first_chunk():
    case = pc.a3_case()
    assert 2 * pc.PP_SCAN < pc.nblk(case.n) <= 3 * pc.PP_SCAN and (case.sd, case.k, case.iters) == (4, 16, (1,))
    f32, dec, _, _ = seeds_of(case)
    for sub in range(case.m):
        rows = sub_rows(case, sub)
        picked = pc.nearest_rows(rows, dec[sub])
        assert (picked < pc.LDS_ROWS).any() and (picked >= pc.LDS_ROWS).any(), (sub, sorted(picked.tolist()))
        # the int8 step is coarser than the spacing of half a million rows: the exact seeds say the same
        exact = np.array([int(np.flatnonzero((rows == c).all(1))[0]) for c in f32[sub]])
        assert (exact[1:] < pc.LDS_ROWS).any() and (exact[1:] >= pc.LDS_ROWS).any(), (sub, sorted(exact.tolist()))
        print("A3 sub-quantizer", sub, "seed rows:", sorted(exact.tolist()))


def test_a4_trains_the_second_sub_quantizer_of_a2():
    case = pc.a4_case()
    assert case.rows() is pc.a2_rows(8) and (case.m, case.sd, case.iters) == (2, 8, (1,))


# ---- B ---------------------------------------------------------------------------------------------------------------------
def test_b_row_counts_sit_on_the_trip_seams():
    for sd in (4, 8, 16):
        t, u = pc.trip_rows(sd), pc.pp_unroll(sd)
        trip_blocks = t // pc.PP_BLOCK
        ns = pc.b_row_counts(sd)
        assert ns == [t - 63, t, t + 1, t + 64 * u + 2, 2 * t + 3, 4 * t + 1]
        blocks = [pc.nblk(n) for n in ns]
        assert blocks[0] == blocks[1] == trip_blocks             # one trip: `more` is never true
        assert blocks[2] == trip_blocks + 1                      # the second trip holds wave 0's first block only
        assert blocks[3] == trip_blocks + u + 1 and ns[3] % pc.PP_BLOCK == 2   # wave 1's first block, two rows
        assert 2 * trip_blocks < blocks[4] <= 3 * trip_blocks    # a third load
        assert blocks[5] == 4 * trip_blocks + 1
        assert {n % pc.ASSIGN_ROWS for n in ns} == {0, 1, 2, 3}  # every tail of pq_assign_vec_kernel's rows per thread
    assert pc.B_GENERIC == [(12, 64 * 16 + 1), (12, 64 * 33 + 7)]
    cases = list(pc.b_cases())
    assert len(cases) == 3 * 6 + 2
    assert all((c.m, c.k, c.iters) == (2, 16, (0, 2)) for c in cases)


@pytest.mark.parametrize("case", list(pc.b_cases()), ids=lambda c: c.name)
def test_b_rows_are_unit_and_lloyd_moves_the_seeds(case):
    x = case.rows()
    assert np.allclose(np.linalg.norm(x.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert_seeds_are_rows(case)
    for sub in range(case.m):
        assert np.unique(seeds_of(case)[0][sub], axis=0).shape[0] == case.k
    opq = o.ProductQuantizer(case.dim, case.m, case.k)
    opq.train(x, iters=2, seed=case.seed)
    assert not np.array_equal(opq.centroids_f32.reshape(case.m, case.k, case.sd), seeds_of(case)[0])


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,big", pc.C_SHAPES)
def test_c_second_seed_is_the_walks_fallback(name, n, big):
    assert pc.fallback_seed(n, big) == pc.C_FOUND[name]        # the lowest seed of the search, well inside 2^26 tries
    case = {c.name: c for c in pc.c_cases()}[name]
    seed, first = pc.C_FOUND[name]
    assert case.seed == seed and (case.m, case.k, case.iters) == (1, 2, (0,))
    assert first == o.rng_u64(seed, 0, 1, 0) % n and first not in (big, n - 1)
    x = case.rows()
    assert not x[first].any() and np.array_equal(x[big], [pc.C_BIG, 0, 0, 0])
    # the picked block: its left-to-right sum from the prefix before it stays below its tree total
    mind = (x.astype(np.float64) ** 2).sum(1).astype(np.float32)          # exact: D^2 against the zero vector
    assert mind[big] == np.float32(2.0 ** 24)
    e0 = big // pc.PP_BLOCK * pc.PP_BLOCK

    def tree(v):
        a = np.zeros(pc.PP_BLOCK, np.float32)
        a[:v.size] = v
        while a.size > 1:
            a = a[0::2] + a[1::2]
        return a[0]
    before = tree(mind[:e0]) if e0 else np.float32(0)
    walked = before
    for v in mind[e0:]:
        walked = np.float32(walked + v)
    assert walked < np.float32(before + tree(mind[e0:]))
    f32, dec, _, _ = seeds_of(case)
    assert np.array_equal(f32[0, 0], x[first])
    assert np.array_equal(f32[0, 1].view(np.uint32), x[n - 1].view(np.uint32))   # the block's last row
    assert not np.array_equal(x[n - 1], x[big]) and dec[0, 1, 0] < 1.0 and abs(dec[0, 1, 0] - 0.875) < 0.01


# ---- D ---------------------------------------------------------------------------------------------------------------------
def test_d_identical_rows_take_the_equal_extremes_branch():
    case = pc.d_identical_case()
    assert (case.n, case.dim, case.m, case.k, case.iters) == (70, 8, 2, 4, (2,))
    x = case.rows()
    assert (x == x[0]).all()
    opq = o.ProductQuantizer(case.dim, case.m, case.k)
    opq.train(x, iters=2, seed=case.seed)
    cent = opq.centroids_f32.reshape(case.m, -1)
    assert (cent.max(1) == cent.min(1)).all()                   # mx == mn in every sub-quantizer
    assert (opq.scales > 0).all() and (opq.scales < 1e-8).all()
    assert (opq.codebooks == -128).all()


def test_d_small_k_cases():
    cases = list(pc.d_small_k_cases())
    assert sorted((c.k, c.sd) for c in cases) == [(k, sd) for k in (1, 2) for sd in (4, 8, 12)]
    for case in cases:
        assert (case.n, case.m, case.iters) == (300, 2, (0, 2))
        assert_seeds_are_rows(case)
        f32 = seeds_of(case)[0]
        for sub in range(case.m):
            first = o.rng_u64(case.seed, sub, 1, 0) % case.n
            assert np.array_equal(f32[sub, 0], sub_rows(case, sub)[first])
            assert case.k == 1 or not np.array_equal(f32[sub, 0], f32[sub, 1])


def test_d_few_distinct_sub_vectors():
    cases = list(pc.d_few_cases())
    assert [c.sd for c in cases] == [4, 16, 12]
    for case in cases:
        assert (case.m, case.k) == (2, 16)
        assert np.unique(sub_rows(case, 1), axis=0).shape[0] == pc.D_FEW_DISTINCT < case.k
        f32 = seeds_of(case)[0]
        assert np.unique(f32[0], axis=0).shape[0] == case.k
        # every distinct sub-vector is a seed, after which the running sum is zero and the rest are repeats
        assert np.unique(f32[1], axis=0).shape[0] == pc.D_FEW_DISTINCT


def test_d_iters0_case_is_the_existing_shape():
    case = pc.d_iters0_case()
    assert (case.n, case.dim, case.m, case.k, case.iters, case.seed) == (1000, 128, 8, 256, (0,), 42)
    rng = np.random.default_rng(1000 + 128 + 8)
    v = rng.standard_normal((1000, 128)).astype(np.float32)
    assert np.array_equal(case.rows(), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))
