"""vg_hnsw_build / vg_hnsw_insert on the cases of tests/hnsw_build_seams.py: the oracle's graph, bit for bit — back-link chains
of hundreds of records on one row, work at lane 0 and lane 63 of a later chunk, tied rows that settle and rows that never do,
ties under Dot and Cosine, ef_construction at its limits.  tests/test_hnsw_build_seams_cpu.py proves from the oracle's event
log that the cases reach all that; the VG_BUILD_DEBUG totals here show which way build_link_kernel took."""
import re

import numpy as np
import pytest

from oracle import oracle as o
from tests import hnsw_build_seams as hs
from tests import hooks
from tests.test_gpu_hnsw_insert import _same_graph, _same_search

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in hs.cases()]
PRUNED, APPENDED, ALREADY = o.LINK_PRUNED, o.LINK_APPENDED, o.LINK_ALREADY
SETTLED = o.LINK_ROW_CHOSEN | o.LINK_FARTHER | o.LINK_UNCHANGED | o.LINK_TIE_MEMBERS


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def _args(c):
    return dict(m=c.m, ef_construction=c.ef, max_batch=c.max_batch, growth_div=c.growth_div)


def _built(vg, ctx, c, rows):
    idx = vg.Index(ctx, rows.shape[0], c.dim, vg.Metric(c.metric))
    idx.set_vectors(rows)
    idx.build_hnsw(**_args(c))
    return idx


@pytest.mark.parametrize("name", NAMES)
def test_build_matches_oracle(vg, ctx, name):
    c = hs.case(name)
    want = hs.oracle_build(name)[:3]
    idx = _built(vg, ctx, c, c.base)
    _same_graph(idx.get_hnsw_graph(), want)
    _same_search(idx, c.base, c.dim, want, c.metric, c.m, np.random.default_rng(len(name)))
    idx.close()


# the cut is a batch boundary of the one-call schedule, and the first batch after it is a chain of hundreds on row 0: the
# hub cases' batch of planted rows (512..811), the cube's first batch of 400
@pytest.mark.parametrize("path", ["built", "uploaded", "uploaded+distances"])
@pytest.mark.parametrize("name,cut", [("hub-m8", 512), ("hub-m32", 512), ("hub-ties-m32", 512), ("swap-m32", 512),
                                      ("cube-m16", 512), ("cube-m32", 512)])
def test_insert_after_a_cut_matches_oracle(vg, ctx, name, cut, path):
    """build_hnsw of the prefix, or the oracle's graph of the prefix uploaded (every row the insert reaches has its state
    derived: row 0 at degree 2M, full, before the chain hits it), then insert_hnsw of the rest: the oracle's graph of all."""
    c = hs.case(name)
    n = c.base.shape[0]
    assert cut in [t0 for t0, _ in hs.batches(n, c.max_batch, c.growth_div)]
    want = hs.oracle_build(name)[:3]
    if path == "built":
        idx = _built(vg, ctx, c, c.base[:cut])
    else:
        l0, upper, ep = o.hnsw_build(c.base[:cut], c.dim, m=c.m, ef=c.ef, metric=c.metric, max_batch=c.max_batch,
                                     growth_div=c.growth_div)
        assert (l0[0] != 0xFFFFFFFF).all()  # row 0 is full in the prefix: cnt = 2M in the derive kernel's pair decode
        idx = vg.Index(ctx, cut, c.dim, vg.Metric(c.metric))
        idx.set_vectors(c.base[:cut])
        idx.set_hnsw_graph(l0, upper, ep, m=c.m)
        if path == "uploaded+distances":
            idx.set_hnsw_edge_distances()
    idx.insert_hnsw(c.base[cut:], **_args(c))
    assert idx.n == n
    _same_graph(idx.get_hnsw_graph(), want)
    _same_search(idx, c.base, c.dim, want, c.metric, c.m, np.random.default_rng(cut))
    idx.close()


TOTALS = re.compile(r"vg_hnsw_build: back links (\d+) = (\d+) skipped \([^;]*; (\d+) of them[^)]*\) \+ (\d+) appended \+ "
                    r"(\d+) pruned; target-row visits that found the row fully chosen (\d+); "
                    r"longest per-row chain in one batch (\d+)")
HUBS = re.compile(r"vg_hnsw_build: rows with >= 1000 back links in a batch: (\d+) visits, (\d+) records of which (\d+) applied")


@pytest.mark.parametrize("name", ["hub-m8", "hub-ties-m32", "chain-1000"])
def test_debug_totals_agree_with_the_event_log(vg, ctx, capfd, name):
    """VG_BUILD_DEBUG: the graph is still the oracle's, and what the link kernel says it did with the records is what the
    oracle's log says could be done with them — `skipped` counts the records that ended in the chunk walk's ballot."""
    c = hs.case(name)
    *want, links, _ = hs.oracle_build(name)
    capfd.readouterr()
    hooks.set_hook("VG_BUILD_DEBUG", 1)
    try:
        idx = _built(vg, ctx, c, c.base)
    finally:
        hooks.set_hook("VG_BUILD_DEBUG", 0)
    err = capfd.readouterr().err
    _same_graph(idx.get_hnsw_graph(), tuple(want))
    idx.close()
    found = TOTALS.findall(err)
    assert len(found) == 1, err[-2000:]
    records, skipped, skipped_stable, appended, pruned, _, longest = (int(v) for v in found[0])
    chains = hs.chains(links)
    on_full = np.count_nonzero(links["outcome"] == PRUNED)
    print(f"{name}: records {records} skipped {skipped} (stable {skipped_stable}) appended {appended} pruned {pruned} "
          f"longest {longest}; log: {len(links)} events, {on_full} on full rows")
    assert records == len(links)
    assert appended == np.count_nonzero(links["outcome"] == APPENDED)
    assert skipped + pruned == on_full and np.count_nonzero(links["outcome"] == ALREADY) == 0
    assert longest == max(len(v) for v in chains.values())
    # only a record that finds a fully chosen row, is strictly farther and leaves it as it was can have been skipped
    may_skip = o.LINK_ROW_CHOSEN | o.LINK_FARTHER | o.LINK_UNCHANGED
    assert 0 < skipped <= np.count_nonzero((links["flags"] & may_skip) == may_skip)
    # `stable`: of a run of such records on a row with tied members, the first takes the long way and proves the row
    # settled; every other one must have been skipped (the row's state starts anew with every batch)
    settled = runs = 0
    for chain in chains.values():
        s = ((chain["flags"] & SETTLED) == SETTLED).astype(np.int8)
        settled += int(s.sum())
        runs += int(np.count_nonzero(np.diff(np.r_[0, s]) == 1))
    assert settled - runs <= skipped_stable <= settled
    # without tied members nothing has to be proven first: every such record is skipped
    plain = np.count_nonzero((links["flags"] & (may_skip | o.LINK_TIE_MEMBERS)) == may_skip)
    assert skipped - skipped_stable == plain
    if name == "hub-ties-m32":
        assert settled >= 500 and skipped_stable >= 500
    hub = HUBS.findall(err)
    assert len(hub) == 1
    visits, hub_records, _ = (int(v) for v in hub[0])
    big = [len(v) for v in chains.values() if len(v) >= 1000]
    assert visits == len(big) and hub_records == sum(big)
    if name == "chain-1000":
        assert visits >= 1
