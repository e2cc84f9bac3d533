"""The seams of k_kmeans.hip, reached on purpose (tests/kmeans_seams.py builds the inputs, tests/test_kmeans_seams_cpu.py
shows they are what they claim): the 32-centroid ranges of the listed points' pass with non-finite and duplicated centroids
at their starts and ends, that pass against the single walk it replaced, km_update_kernel at the cluster sizes where its
loop changes shape and on an empty cluster, the member sort's scan carry, its smallest and largest LDS k and the first k
past it, and both branches of vg_find_closest_centroids.  Every expected value is the oracle's; assignments compare as
int32, centroids as bit patterns."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import kmeans_seams as ks
from tests.hooks import set_hook

pytestmark = pytest.mark.gpu


def bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


@pytest.fixture(scope="module")
def seam_cases():
    """[(name, x, c, metric, the oracle's assignment)]: computed once, shared and left unchanged."""
    out = []
    for name, x, c, metric in list(ks.nan_seam_cases()) + list(ks.clean_seam_cases()):
        want = o.assign_partition_batch(x, c, metric)
        want.setflags(write=False)
        out.append((name, x, c, metric, want))
    return out


def assert_assignment(got, want, label):
    got = np.asarray(got)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (label, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def test_non_finite_and_tied_centroids_on_range_seams(vg, ctx, seam_cases):
    for hook in (None, "VG_KM_LIST_ALL", "VG_KM_BF16"):
        if hook:
            set_hook(hook, 1)
        try:
            for name, x, c, metric, want in seam_cases:
                if name.startswith("clean"):
                    continue
                assert_assignment(vg.kmeans_assign(ctx, x, c, x.shape[1], metric), want, (name, hook))
        finally:
            if hook:
                set_hook(hook, 0)


def test_ranged_pass_equals_the_single_walk(vg, ctx, seam_cases):
    set_hook("VG_KM_LIST_ALL", 1)
    try:
        for name, x, c, metric, want in seam_cases:
            ranged = np.asarray(vg.kmeans_assign(ctx, x, c, x.shape[1], metric))
            set_hook("VG_KM_NO_RANGES", 1)
            try:
                walk = np.asarray(vg.kmeans_assign(ctx, x, c, x.shape[1], metric))
            finally:
                set_hook("VG_KM_NO_RANGES", 0)
            assert_assignment(walk, want, (name, "single walk"))
            assert_assignment(ranged, want, (name, "ranged"))
            assert np.array_equal(walk, ranged), name
    finally:
        set_hook("VG_KM_NO_RANGES", 0)
        set_hook("VG_KM_LIST_ALL", 0)


# dim 8, 1416 rows: the reference-order assignment; dim 64 with filler groups up to 4116 rows: the matrix path (bfloat16
# splits from three iterations) — the sorted member lists and km_update_kernel's three shapes in both
@pytest.mark.parametrize("dim,sizes", [(8, ks.UPDATE_SIZES), (64, ks.UPDATE_SIZES + [700, 900, 1100])])
def test_update_at_queue_depth_seams(vg, ctx, dim, sizes):
    seed = 11
    x = ks.planted_clusters(sizes, dim, seed)
    k = len(sizes)
    assert x.shape[0] >= 4096 or dim == 8
    for metric in (0, 2):
        for max_iter in (1, 2, 5):   # 1: the first update alone; later: the reseeded centroid takes members
            exp = o.kmeans_train(x, dim, k, metric, max_iter, seed=seed)
            got = vg.kmeans_train(ctx, x, dim, k, metric, max_iter, seed=seed)
            bad = np.nonzero(bits(got) != bits(exp))[0]
            assert bad.size == 0, (metric, max_iter, np.unique(bad // dim), [sizes[c] for c in np.unique(bad // dim)])


@pytest.mark.parametrize("n,dim,k,iters", [(530_000, 8, 3, 2),     # 259 parts of 2048 rows: the scan carries across 256
                                           (5000, 8, 1, 2),        # no bit of the cluster id to ballot on
                                           (4200, 8, 4096, 2),     # the last k with LDS counters
                                           (4200, 8, 4097, 2),     # the first k without
                                           (3000, 16, 64, 3), (3000, 16, 65, 3)])   # a power of two and the next k
def test_member_sort_seams(vg, ctx, n, dim, k, iters):
    rng = np.random.default_rng(n + dim + k)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    exp = o.kmeans_train(x, dim, k, 0, iters, seed=11)
    got = vg.kmeans_train(ctx, x, dim, k, 0, iters, seed=11)
    bad = np.nonzero(bits(got) != bits(exp))[0]
    assert bad.size == 0, (bad.size, np.unique(bad // dim)[:8])


@pytest.mark.parametrize("k,nprobes", [(40, (9, 10, 11, 15, 16, 40, 50)), (64, (15, 16, 17))])
@pytest.mark.parametrize("metric", [0, 2])
def test_find_closest_centroids_across_the_sort_switch(vg, ctx, k, nprobes, metric):
    """Selection loop for nprobe <= k / 4 and nprobe < 16, full sort otherwise.  The reference's sort leaves ties unpinned:
    the distances are distinct before anything is compared."""
    dim = 16
    rng = np.random.default_rng(100 * k + metric)
    cc = rng.standard_normal((k, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    d = o.l2_batch(q, cc, dim) if metric == 0 else o.dot_batch(q, cc, dim)
    assert np.unique(d).size == k and np.isfinite(d).all()
    branches = set()
    for nprobe in nprobes:
        n = min(nprobe, k)
        branches.add(n <= k // 4 and n < 16)
        want = o.find_closest_centroids(q, cc, dim, nprobe, metric)
        assert want.size == n
        assert np.array_equal(want, np.argsort(d if metric == 0 else -d, kind="stable")[:n])
        got = vg.find_closest_centroids(ctx, q, cc, dim, nprobe, metric)
        assert np.array_equal(np.asarray(got), want), (nprobe, got, want)
    assert branches == {True, False}
