"""Training sets that put the seams of ProductQuantizer Train's k-means++ seeding (k_pq_train.hip: pq_kmeanspp_kernel) under
the data instead of leaving them to chance: block prefixes that leave LDS and are scanned in carried chunks, the trip
seams of the software-pipelined distance pass and the row tail of pq_assign_vec_kernel, a block whose tree total
exceeds its sequential sum (the walk's fallback), and the degenerate inputs of pq_quantize_kernel and of small k.

Plain numpy builders, each with its own generator: tests/test_pq_train_cases_cpu.py checks them against the oracle
alone, tests/test_gpu_pq_train_seams.py runs the library on them."""
import functools
import re
from pathlib import Path
from typing import Callable, NamedTuple, Tuple

import numpy as np

from oracle import oracle as o

_SRC = (Path(__file__).resolve().parent.parent / "vecgo_amd" / "csrc" / "k_pq_train.hip").read_text()
PP_THREADS = int(re.search(r"kPPThreads = (\d+);", _SRC).group(1))
PP_BLOCK = int(re.search(r"kPPBlock = (\d+);", _SRC).group(1))    # rows per block total
PP_SCAN = int(re.search(r"kPPScan = (\d+);", _SRC).group(1))      # block totals per scan chunk
ASSIGN_ROWS = int(re.search(r"kAssignRows = (\d+);", _SRC).group(1))
UNROLL_RULE = "kPPUnroll = SD >= 16 ? 2 : (SD >= 8 ? 3 : 4);"   # test_pq_train_cases_cpu.py: still the kernel's line
LDS_ROWS = PP_BLOCK * PP_SCAN                                      # the last row count whose prefixes stay in LDS


def pp_unroll(sd):
    """Blocks per wave and trip of the templated distance pass."""
    return 2 if sd >= 16 else (3 if sd >= 8 else 4)


def trip_rows(sd):
    """Rows the workgroup covers in one trip: kTrip = 16 kPPUnroll blocks of 64."""
    return (PP_THREADS // 64) * pp_unroll(sd) * PP_BLOCK


def nblk(n):
    return (n + PP_BLOCK - 1) // PP_BLOCK


class Case(NamedTuple):
    name: str
    rows: Callable[[], np.ndarray]    # () -> float32 [n, m * sd], read-only
    n: int
    sd: int
    m: int
    k: int
    iters: Tuple[int, ...]
    seed: int

    @property
    def dim(self):
        return self.m * self.sd


def _frozen(x):
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


def unit_vectors(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


# ---- A: prefixes in global memory ---------------------------------------------------------------------------------------
A_M, A_K = 2, 8
A2_HEAD, A2_TAIL = LDS_ROWS, 16 * PP_BLOCK + 1         # 17 blocks behind the first chunk, the last one of one row
A3_N = 2 * LDS_ROWS + PP_BLOCK * 17 + 5
A3_SD, A3_K = 4, 16


@functools.lru_cache(maxsize=1)
def a1_rows():
    """LDS_ROWS + 1 iid normal rows; the LDS_ROWS case takes all but the last."""
    return _frozen(np.random.default_rng(21).standard_normal((LDS_ROWS + 1, A_M * 8)))


@functools.lru_cache(maxsize=2)
def a2_rows(sd):
    """A light head that fills the first scan chunk and a heavy tail behind it, of comparable D^2 mass; coordinate 0 of
    every sub-vector is negative in the head and positive in the tail, at least 0.5 either way."""
    rng = np.random.default_rng(5)
    dim = A_M * sd
    head = rng.standard_normal((A2_HEAD, dim)) * 0.25
    tail = rng.standard_normal((A2_TAIL, dim)) * 4.0
    head[:, ::sd] = -(0.5 + rng.random((A2_HEAD, A_M)) / 2)
    tail[:, ::sd] = 0.5 + rng.random((A2_TAIL, A_M)) / 2
    return _frozen(np.concatenate([head, tail]))


@functools.lru_cache(maxsize=1)
def a3_rows():
    return _frozen(np.random.default_rng(31).standard_normal((A3_N, A_M * A3_SD)))


def a1_cases():
    for n in (LDS_ROWS, LDS_ROWS + 1):
        yield Case(f"A1-n{n}", functools.partial(lambda n: a1_rows()[:n], n), n, 8, A_M, A_K, (0, 1), 1)


def a2_cases():
    for sd in (4, 8, 16, 12):
        yield Case(f"A2-sd{sd}", functools.partial(a2_rows, sd), A2_HEAD + A2_TAIL, sd, A_M, A_K, (0, 1), 1)


def a3_case():
    return Case("A3-three-chunks", a3_rows, A3_N, A3_SD, A_M, A3_K, (1,), 1)


def a4_case():
    """A2's sd = 8 rows; the test trains sub-quantizer 1 alone."""
    return Case("A4-subset", functools.partial(a2_rows, 8), A2_HEAD + A2_TAIL, 8, A_M, A_K, (1,), 1)


# ---- B: trip seams of the distance pass, row tail of the assignment ---------------------------------------------------------
B_M, B_K = 2, 16


def b_row_counts(sd):
    t = trip_rows(sd)
    return [t - 63,                                # the last block of the one trip is ragged
            t,
            t + 1,                                 # a second trip in which only wave 0 has work
            t + PP_BLOCK * pp_unroll(sd) + 2,      # wave 1's first block of the second trip is ragged
            2 * t + 3,                             # a third load: the first register set is reused
            4 * t + 1]


B_GENERIC = [(12, PP_BLOCK * 16 + 1), (12, PP_BLOCK * 33 + 7)]    # around one block per wave and two


@functools.lru_cache(maxsize=None)
def _b_rows(sd, n):
    return _frozen(unit_vectors(np.random.default_rng(1000 * sd + n), n, B_M * sd))


def b_cases():
    shapes = [(sd, n) for sd in (4, 8, 16) for n in b_row_counts(sd)] + B_GENERIC
    for sd, n in shapes:
        yield Case(f"B-sd{sd}-n{n}", functools.partial(_b_rows, sd, n), n, sd, B_M, B_K, (0, 2), 42)


# ---- C: the walk's fallback ------------------------------------------------------------------------------------------------
_U = np.uint64


def _splitmix64(x):
    x = x + _U(0x9e3779b97f4a7c15)
    x = (x ^ (x >> _U(30))) * _U(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> _U(27))) * _U(0x94d049bb133111eb)
    return x ^ (x >> _U(31))


def rng_u64_np(seeds, a, b, c):
    """oracle.rng_u64 over an array of seeds (uint64 arithmetic wraps)."""
    h = _splitmix64(np.asarray(seeds, _U))
    for v in (a, b, c):
        h = _splitmix64(h ^ _U(v))
    return h


C_BIG = 4096.0            # D^2 against the zero vector: 2^24, where one float32 step is 2
C_SD, C_K = 4, 2
C_SHAPES = [("C1-whole-block", 64, 0), ("C2-ragged-block", 50, 0), ("C3-second-block", 128, 64)]   # (name, n, the big row)
C_SEARCH = 1 << 26
# (train seed, the first seed's row) per shape: what fallback_seed() finds, written down so that listing the cases
# searches nothing (test_pq_train_cases_cpu.py runs the search and compares)
C_FOUND = {"C1-whole-block": (156712, 10), "C2-ragged-block": (2302329, 4), "C3-second-block": (156712, 10)}


def fallback_rows(n, big, first):
    """Row `first` (the first seed) is the zero vector and row `big` is (4096, 0, 0, 0); every other row i is
    (0.875, i / 1024, 0, 0), of D^2 about 0.77: added one at a time to 2^24 each rounds away, added to each other first
    (the tree of the block total) they do not."""
    x = np.zeros((n, C_SD), np.float32)
    x[:, 0] = 0.875
    x[:, 1] = np.arange(n, dtype=np.float32) / np.float32(1024)
    x[big] = 0
    x[big, 0] = C_BIG
    x[first] = 0
    return x


def oracle_seeds(x, sd, m, k, seed):
    """The oracle's k-means++ seeds, before any Lloyd iteration: float32 [m, k, sd]."""
    opq = o.ProductQuantizer(m * sd, m, k)
    opq.train(x, iters=0, seed=seed)
    return opq.centroids_f32.reshape(m, k, sd).copy()


@functools.lru_cache(maxsize=None)
def fallback_seed(n, big):
    """The lowest train seed >= 1 for which the oracle's second pick on fallback_rows ends in the walk's fallback, with
    the first seed neither the big row nor the block's last: (seed, first), or None if there is none below C_SEARCH.
    Candidates: the target's 24 random bits within 128 of 2^24 (the sum is about 2^24 + 48 n / 64)."""
    last = n - 1
    step = 1 << 20
    with np.errstate(over="ignore"):
        for lo in range(0, C_SEARCH, step):
            seeds = np.arange(max(lo, 1), lo + step, dtype=_U)
            first = rng_u64_np(seeds, 0, 1, 0) % _U(n)
            top = rng_u64_np(seeds, 0, 1, 1) >> _U(40)
            keep = (top >= _U((1 << 24) - 128)) & (first != _U(big)) & (first != _U(last))
            for s, f in zip(seeds[keep].tolist(), first[keep].tolist()):
                x = fallback_rows(n, big, f)
                second = oracle_seeds(x, C_SD, 1, C_K, s)[0, 1]
                if np.array_equal(second, x[last]):
                    return s, f
    return None


def c_cases():
    for name, n, big in C_SHAPES:
        seed, first = C_FOUND[name]
        yield Case(name, functools.partial(lambda n, big, first: _frozen(fallback_rows(n, big, first)), n, big, first),
                   n, C_SD, 1, C_K, (0,), seed)


# ---- D: degenerate inputs --------------------------------------------------------------------------------------------------
def _identical_rows():
    """70 copies of one row whose sub-vectors are constant: every centroid coordinate of a sub-quantizer is the same number."""
    return _frozen(np.tile(np.repeat(np.array([1.5, -0.25], np.float32), 4), (70, 1)))


@functools.lru_cache(maxsize=None)
def _small_k_rows(sd):
    return _frozen(np.random.default_rng(400 + sd).standard_normal((300, 2 * sd)))


D_FEW_DISTINCT, D_FEW_K = 5, 16


@functools.lru_cache(maxsize=None)
def _few_rows(sd):
    """Sub-quantizer 0 sees 300 random sub-vectors, sub-quantizer 1 only D_FEW_DISTINCT (< k), repeated."""
    rng = np.random.default_rng(500 + sd)
    x = rng.standard_normal((300, 2 * sd)).astype(np.float32)
    pool = rng.standard_normal((D_FEW_DISTINCT, sd)).astype(np.float32)
    x[:, sd:] = pool[np.arange(300) % D_FEW_DISTINCT]
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def _pq_test_rows():
    """The (1000, 128, 8, 256) rows of test_gpu_pq.py's Train comparison."""
    return _frozen(unit_vectors(np.random.default_rng(1000 + 128 + 8), 1000, 128))


def d_identical_case():
    return Case("D-identical", _identical_rows, 70, 4, 2, 4, (2,), 9)


def d_small_k_cases():
    for k in (1, 2):
        for sd in (4, 8, 12):
            yield Case(f"D-k{k}-sd{sd}", functools.partial(_small_k_rows, sd), 300, sd, 2, k, (0, 2), 7)


def d_few_cases():
    for sd in (4, 16, 12):
        yield Case(f"D-few-sd{sd}", functools.partial(_few_rows, sd), 300, sd, 2, D_FEW_K, (0, 3), 9)


def d_iters0_case():
    return Case("D-iters0-1000x128", _pq_test_rows, 1000, 16, 8, 256, (0,), 42)


def all_cases():
    """Every case the GPU test trains in full (A4 trains a range and is run on its own)."""
    yield from a1_cases()
    yield from a2_cases()
    yield a3_case()
    yield from b_cases()
    yield from c_cases()
    yield d_identical_case()
    yield from d_small_k_cases()
    yield from d_few_cases()
    yield d_iters0_case()


# ---- reading a codebook back -----------------------------------------------------------------------------------------------
def decode(codebooks, scales, offsets, m, k, sd):
    """float32 [m, k, sd] centroids as Decode forms them: two rounded float32 operations (pq.go:205-215)."""
    cb = np.asarray(codebooks, np.int8).reshape(m, k, sd).astype(np.float32)
    step = (cb * np.asarray(scales, np.float32)[:, None, None]).astype(np.float32)
    return (step + np.asarray(offsets, np.float32)[:, None, None]).astype(np.float32)


def nearest_rows(sub_rows, cent):
    """Index of the row of sub_rows [n, sd] nearest to each centroid of cent [k, sd] (float64)."""
    rows = sub_rows.astype(np.float64)
    return np.array([int(((rows - c.astype(np.float64)) ** 2).sum(1).argmin()) for c in cent])
