"""The Vamana builders' split of a batch's visited bitmaps over several launches (VamanaBatch::search, vg_vamana_common.hpp):
under the test hook VG_VAMANA_SMALL_SCRATCH a launch's bitmaps get 64 KiB, so a batch of 512 nodes over a few thousand rows
walks in three or four launches, the last one ragged.  vg_vamana_build, vg_vamana_insert and vg_vamana_consolidate with the
hook on must leave what they leave with it off, bit for bit: every node searches the graph as it stood when its batch began,
whichever launch carries it.  (The hook-off side of these shapes is the code the parity tests pin to the sequential
restatements at smaller n.)"""
import numpy as np
import pytest

from tests.hooks import set_hook

pytestmark = pytest.mark.gpu

DIM, R, L, ALPHA, MAX_BATCH = 16, 8, 20, 1.2, 512
N_BUILD, N_INSERT = 3000, 1000
CAP = 65536  # the hook's bytes of bitmaps per launch


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


@pytest.fixture(scope="module")
def rows():
    return np.random.default_rng(5).standard_normal((N_BUILD + N_INSERT, DIM)).astype(np.float32)


def _launches(n, batch):
    """the launches a batch of `batch` nodes takes over n rows under the hook, from the driver's arithmetic"""
    per_launch = CAP // (4 * -(-n // 32))
    return [min(per_launch, batch - c0) for c0 in range(0, batch, per_launch)]


def _largest_batch(done, end, growth_div):
    """the largest batch of the schedule clamp(done / growth_div, 1, MAX_BATCH) from `done` nodes to `end`"""
    largest = 0
    while done < end:
        b = min(max(1, min(done // growth_div, MAX_BATCH)), end - done)
        largest, done = max(largest, b), done + b
    return largest


def _built(vg, ctx, rows):
    idx = vg.Index(ctx, N_BUILD, DIM, vg.Metric(0))
    idx.set_vectors(rows[:N_BUILD])
    idx.build_vamana(r=R, l=L, alpha=ALPHA, seed=5, max_batch=MAX_BATCH, growth_div=2)
    return idx


def _inserted(vg, ctx, rows, graph, entry):
    idx = vg.Index(ctx, N_BUILD, DIM, vg.Metric(0))
    idx.set_vectors(rows[:N_BUILD])
    idx.set_vamana_graph(graph, entry)
    idx.insert_vamana(rows[N_BUILD:], r=R, l=L, alpha=ALPHA, max_batch=MAX_BATCH, growth_div=1)
    return idx


def _hooked(fn):
    set_hook("VG_VAMANA_SMALL_SCRATCH", 1)
    try:
        return fn()
    finally:
        set_hook("VG_VAMANA_SMALL_SCRATCH", 0)


@pytest.fixture(scope="module")
def whole(vg, ctx, rows):
    """hook off, computed once: the built graph, the graph after the insert (each with its entry point)"""
    idx = _built(vg, ctx, rows)
    built = idx.get_vamana_graph()
    idx.close()
    idx = _inserted(vg, ctx, rows, *built)
    grown = idx.get_vamana_graph()
    idx.close()
    return built, grown


def _same(got, want):
    assert got[1] == want[1]
    bad = np.nonzero((got[0] != want[0]).any(1))[0]
    assert got[0].shape == want[0].shape and bad.size == 0, (bad[:5], got[0][bad[0]], want[0][bad[0]])


def test_build(vg, ctx, rows, whole):
    # growth_div 2: the batches grow to 512 within the first of the two passes
    assert _largest_batch(0, N_BUILD, 2) == MAX_BATCH and _launches(N_BUILD, MAX_BATCH) == [174, 174, 164]
    idx = _hooked(lambda: _built(vg, ctx, rows))
    _same(idx.get_vamana_graph(), whole[0])
    idx.close()


def test_insert(vg, ctx, rows, whole):
    # growth_div 1: a batch is as large as the graph before it, capped at 512: 512 + 488 new rows
    assert _largest_batch(N_BUILD, N_BUILD + N_INSERT, 1) == MAX_BATCH
    assert _launches(N_BUILD + N_INSERT, MAX_BATCH) == [131, 131, 131, 119]
    idx = _hooked(lambda: _inserted(vg, ctx, rows, *whole[0]))
    _same(idx.get_vamana_graph(), whole[1])
    assert idx.n == N_BUILD + N_INSERT
    idx.close()


def test_consolidate(vg, ctx, rows, whole):
    n = N_BUILD + N_INSERT
    deleted = np.zeros(n, bool)
    deleted[::10] = True

    def run():
        idx = vg.Index(ctx, n, DIM, vg.Metric(0))
        idx.set_vectors(rows)
        idx.set_vamana_graph(*whole[1])
        stats = idx.consolidate_vamana(deleted, l=L, alpha=ALPHA, max_batch=MAX_BATCH)
        out = idx.get_vamana_graph()
        idx.close()
        return out, stats

    want, want_stats = run()
    got, got_stats = _hooked(run)
    assert set(want_stats) == {"repaired_nodes", "dropped_links", "links_before", "links_after"}
    assert got_stats == want_stats, (got_stats, want_stats)
    largest = min(MAX_BATCH, want_stats["repaired_nodes"])
    assert want_stats["repaired_nodes"] > 131 and len(_launches(n, largest)) > 1  # a batch of the repair really splits
    _same(got, want)
    assert not np.array_equal(want[0], whole[1][0])  # and the repair rewrote lists
