"""Inputs that put the seams of k_kmeans.hip under the data instead of leaving them to chance: the 32-centroid ranges of the
listed points' pass (km_assign_regs_kernel<.., LIST>), and the cluster sizes at which km_update_kernel changes shape.

Plain builders: tests/test_kmeans_seams_cpu.py checks them against the oracle alone, tests/test_gpu_kmeans_seams.py runs the
library on them."""
import functools

import numpy as np

from oracle import oracle as o

SEAM_N = 4099                 # odd, just above the 4096 rows from which the matrix path (and so the listed pass) serves
SEAM_SHAPES = [(dim, k) for dim in (64, 128) for k in (33, 64, 65, 97)] + [(768, 97)]
# the sizes around km_update_kernel's 64-deep register queue (tail only / fill and drain / steady loop + tail), an empty
# cluster (the reseed) and a few others
UPDATE_SIZES = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 0, 2, 256, 5]


@functools.lru_cache(maxsize=None)
def _seam_base(dim, k):
    rng = np.random.default_rng(1000 * dim + k)
    x = rng.standard_normal((SEAM_N, dim)).astype(np.float32)
    c = x[rng.choice(SEAM_N, k, replace=False)].copy()
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c


def _centroid_edits(c):
    """(name, edited copy) for every edit the centroid count allows.  Ranges are 32 centroids: 32 and 64 start one, 31 ends
    one."""
    k, dim = c.shape
    col = 5 % dim

    def edit(name, fn):
        e = c.copy()
        fn(e)
        return name, e

    def put(index, value, column=col):
        def fn(e):
            for i in np.atleast_1d(index):
                if column is None:
                    e[i] = value
                else:
                    e[i, column] = value
        return fn

    yield edit("nan32", put(32, np.nan))
    if k >= 65:
        yield edit("nan64", put(64, np.nan))
    yield edit("nan31", put(31, np.nan))
    yield edit("nan0+32", put([0, 32], np.nan))
    if k >= 65:
        yield edit("nan32..63", put(np.arange(32, 64), np.nan, None))
    yield edit("+inf32", put(32, np.inf, None))
    yield edit("-inf32", put(32, -np.inf, None))

    def ties(e):             # exact ties across a range boundary: the lowest index wins
        e[32] = e[31]
        if k >= 65:
            e[64] = e[5]
    yield edit("ties", ties)


def nan_seam_cases():
    """(name, x, c, metric): non-finite and duplicated centroids at the starts and ends of the 32-centroid ranges, and one
    case of NaN rows with clean centroids.  x is shared between the cases of a shape and read-only."""
    for dim, k in SEAM_SHAPES:
        x, c = _seam_base(dim, k)
        for ename, ce in _centroid_edits(c):
            for metric in (0, 2):
                yield f"{ename}-d{dim}-k{k}-m{metric}", x, ce, metric
    x, c = _seam_base(64, 97)
    xn = x.copy()
    xn[[0, 17, 2048, SEAM_N - 1], [3, 0, 63, 31]] = np.nan
    xn[100] = np.nan
    for metric in (0, 2):
        yield f"nanrows-d64-k97-m{metric}", xn, c.copy(), metric


def clean_seam_cases():
    """Two clean random cases for the ranged pass against the single walk: (name, x, c, metric)."""
    for n, dim, k in ((4099, 64, 97), (4100, 768, 130)):
        rng = np.random.default_rng(n + dim + k)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        c = x[rng.choice(n, k, replace=False)].copy()
        for metric in (0, 2):
            yield f"clean-n{n}-d{dim}-k{k}-m{metric}", x, c, metric


def nan_centroids(c):
    """Indices of the centroids that hold a NaN."""
    return np.nonzero(np.isnan(c).any(axis=1))[0]


def initial_rows(n, k, seed):
    """The rows vg_kmeans_train takes as its k initial centroids: the first k entries of its partial Fisher-Yates shuffle."""
    perm = np.arange(n, dtype=np.int64)
    for i in range(min(k, n - 1)):
        j = i + o.rng_u64(seed, 0, 1, i) % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return perm[:k]


def planted_clusters(sizes, dim, seed):
    """float32 [sum(sizes), dim] rows on which the first Lloyd pass of a k = len(sizes) training run with `seed` gives cluster
    j exactly sizes[j] members, under L2 and under the dot metrics.

    Group j's centre sits on the row that becomes initial centroid j; its other members are centre + 0.01 N(0, 1) and lie on
    the remaining rows in a shuffled order.  The centres are N(0, 50^2) directions scaled to one common norm (50 sqrt(dim)),
    so the nearest centre and the centre of largest dot product are the same one.  A size of 0 makes the group's centre row a
    bit-exact copy of the centre of the first lower-numbered group of two or more: the tie goes to the lower index, so the
    group gets no member and takes the reseed, and its centre row is one of the lower group's sizes[] members (that group has
    one noisy member fewer)."""
    sizes = list(sizes)
    k = len(sizes)
    n = sum(sizes)
    rng = np.random.default_rng(seed * 7919 + dim)
    centres = rng.standard_normal((k, dim)) * 50.0
    centres *= 50.0 * np.sqrt(dim) / np.linalg.norm(centres, axis=1, keepdims=True)
    centres = centres.astype(np.float32)
    noisy = [s - 1 for s in sizes]           # members besides the centre row
    for j, s in enumerate(sizes):
        if s == 0:
            t = next(t for t in range(j) if noisy[t] >= 1)
            centres[j] = centres[t]
            noisy[t] -= 1
            noisy[j] = 0
    first = initial_rows(n, k, seed)
    x = np.empty((n, dim), np.float32)
    x[first] = centres
    rest = np.setdiff1d(np.arange(n), first)
    rng.shuffle(rest)
    group = np.repeat(np.arange(k), noisy)
    assert group.size == rest.size
    x[rest] = centres[group] + np.float32(0.01) * rng.standard_normal((rest.size, dim)).astype(np.float32)
    return x
