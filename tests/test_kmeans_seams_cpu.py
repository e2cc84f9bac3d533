"""tests/kmeans_seams.py against the oracle alone: the conditions under which tests/test_gpu_kmeans_seams.py cannot pass
vacuously — the reference really skips a NaN centroid at a range start and still assigns into the rest of that range, and the
planted training sets really have the cluster sizes they prescribe."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import kmeans_seams as ks


def test_reference_skips_only_the_nan_centroid():
    seen = 0
    for name, x, c, metric in ks.nan_seam_cases():
        bad = ks.nan_centroids(c)
        bad = bad[bad > 0]
        if bad.size == 0:
            continue
        a = o.assign_partition_batch(x, c, metric)
        assert a.shape == (x.shape[0],)
        assert not np.isin(a, bad).any(), name
        seen += 1
        if name.startswith("nan32-") and c.shape[0] >= 64:
            # the rest of the range that starts with the NaN centroid keeps its rows
            inside = np.count_nonzero((a >= 33) & (a <= 63))
            assert inside >= 0.05 * x.shape[0], (name, inside)
    assert seen >= 2 * 4 * len(ks.SEAM_SHAPES)   # nan32, nan31, nan0+32 (and more from k = 65) per shape and metric


def test_nan_at_a_range_start_changes_only_its_own_rows():
    x, c = ks._seam_base(64, 97)
    clean = o.assign_partition_batch(x, c, 0)
    cases = {name: (cx, cc) for name, cx, cc, metric in ks.nan_seam_cases() if name == "nan32-d64-k97-m0"}
    _, cn = cases["nan32-d64-k97-m0"]
    a = o.assign_partition_batch(x, cn, 0)
    moved = a != clean
    assert np.array_equal(moved, clean == 32) and moved.any()


def test_case_list_covers_what_it_names():
    names = [name for name, *_ in ks.nan_seam_cases()]
    assert len(names) == len(set(names))
    for dim, k in ks.SEAM_SHAPES:
        for edit in ("nan32", "nan31", "nan0+32", "+inf32", "-inf32", "ties"):
            for metric in (0, 2):
                assert f"{edit}-d{dim}-k{k}-m{metric}" in names
        for edit in ("nan64", "nan32..63"):
            assert (f"{edit}-d{dim}-k{k}-m0" in names) == (k >= 65)
    assert "nanrows-d64-k97-m0" in names and "nanrows-d64-k97-m2" in names
    for name, x, c, metric in ks.nan_seam_cases():
        assert x.shape[0] == ks.SEAM_N and x.dtype == c.dtype == np.float32 and c.shape[1] == x.shape[1]
        if name.startswith("ties"):
            assert np.array_equal(c[32], c[31]) and (c.shape[0] < 65 or np.array_equal(c[64], c[5]))


@pytest.mark.parametrize("dim,sizes", [(8, ks.UPDATE_SIZES), (64, ks.UPDATE_SIZES + [700, 900, 1100])])
@pytest.mark.parametrize("metric", [0, 2])
def test_planted_clusters_have_the_prescribed_sizes(dim, sizes, metric):
    seed = 11
    x = ks.planted_clusters(sizes, dim, seed)
    k = len(sizes)
    assert x.shape == (sum(sizes), dim)
    c0 = o.kmeans_train(x, dim, k, metric, 0, seed=seed).reshape(k, dim)
    assert np.array_equal(c0.view(np.uint32), x[ks.initial_rows(x.shape[0], k, seed)].view(np.uint32))
    counts = np.bincount(o.assign_partition_batch(x, c0, metric), minlength=k)
    assert np.array_equal(counts, sizes), counts
    assert {0, 1, 63, 64, 65, 127, 128, 129} <= set(counts.tolist())
    # the empty cluster's reseed is a row of x, and the run goes on moving centroids after the first update
    c1 = o.kmeans_train(x, dim, k, metric, 1, seed=seed).reshape(k, dim)
    empty = sizes.index(0)
    row = o.rng_u64(seed, 0, 2, empty) % x.shape[0]
    assert np.array_equal(c1[empty].view(np.uint32), x[row].view(np.uint32))
    if metric == 0:  # (under the dot metrics a tight group follows the reseeded row as a whole or not at all)
        c2 = o.kmeans_train(x, dim, k, metric, 2, seed=seed).reshape(k, dim)
        assert not np.array_equal(c1.view(np.uint32), c2.view(np.uint32))
