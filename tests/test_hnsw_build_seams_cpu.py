"""tests/hnsw_build_seams.py against the oracle alone: the event log of the oracle's build (one entry per addConnection
call) shows that every case reaches what it is named for, so tests/test_gpu_hnsw_build_seams.py cannot pass vacuously.
These are conditions on the inputs: where one does not hold, the generator is what has to change."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import hnsw_build_seams as hs

ALREADY, APPENDED, PRUNED = o.LINK_ALREADY, o.LINK_APPENDED, o.LINK_PRUNED
TIE, TIE_MEMBERS, FARTHER, UNCHANGED = o.LINK_TIE_ANY, o.LINK_TIE_MEMBERS, o.LINK_FARTHER, o.LINK_UNCHANGED
TIE_LAST, CHOSEN = o.LINK_TIE_LAST, o.LINK_ROW_CHOSEN
NAMES = [c.name for c in hs.cases()]


def _has(ev, flags, none=0):
    return (ev["outcome"] == PRUNED) & ((ev["flags"] & flags) == flags) & ((ev["flags"] & none) == 0)


def _changes(ev):
    """records that leave the row other than they found it"""
    return (ev["outcome"] == APPENDED) | _has(ev, 0, none=UNCHANGED)


def _skippable(ev):
    """a fully chosen row, a strictly farther newcomer, the row as it was: what build_link_kernel may skip"""
    return _has(ev, CHOSEN | FARTHER | UNCHANGED)


def _row0(name):
    """row 0's layer-0 chains of the case, by batch"""
    links = hs.oracle_build(name)[3]
    return {k[0]: v for k, v in hs.chains(links).items() if k[1] == 0 and k[2] == 0}


def test_names_are_distinct_and_rows_frozen():
    assert len(NAMES) == len(set(NAMES))
    for c in hs.cases():
        assert c.base.dtype == np.float32 and not c.base.flags.writeable and c.base.shape[1] == c.dim
        assert c.base.shape[0] <= 2500 and c.dim <= 64


def test_the_log_changes_nothing_and_is_in_application_order():
    c = hs.case("hub-ties-m8")
    plain = o.hnsw_build(c.base, c.dim, m=c.m, ef=c.ef, metric=c.metric, max_batch=c.max_batch, growth_div=c.growth_div)
    l0, upper, entry, links, own = hs.oracle_build(c.name)
    assert entry == plain[2] and np.array_equal(l0, plain[0]) and len(upper) == len(plain[1])
    for (sa, aa), (sb, ab) in zip(upper, plain[1]):
        assert np.array_equal(sa, sb) and np.array_equal(aa, ab)
    # batches in order, and inside a batch ascending id of the new node: the order the link kernel sorts a row's records into
    assert np.all(np.diff(links["batch"]) >= 0)
    same_batch = np.diff(links["batch"]) == 0
    assert np.all(np.diff(links["new_node"].astype(np.int64))[same_batch] >= 0)
    sched = hs.batches(c.base.shape[0], c.max_batch, c.growth_div)
    t0 = np.array([b[0] for b in sched])[links["batch"]]
    size = np.array([b[1] for b in sched])[links["batch"]]
    assert np.all((links["new_node"] >= t0) & (links["new_node"] < t0 + size))
    assert np.all(links["node"] < t0)  # no member of a batch links to another: `already connected` cannot happen in a build
    for chain in hs.chains(links).values():
        assert np.array_equal(chain["pos"], np.arange(len(chain)))
        assert np.all(np.diff(chain["new_node"].astype(np.int64)) > 0)
    assert np.all(links["deg"] == np.where(links["level"] == 0, 2 * c.m, c.m))
    assert np.all((links["flags"] == 0) | (links["outcome"] == PRUNED))
    # one own row per (node, level), every node but the first
    assert np.array_equal(np.unique(own["node"]), np.arange(1, c.base.shape[0]))
    assert np.all(own["kept"] <= np.where(own["level"] == 0, 2 * c.m, c.m))


@pytest.mark.parametrize("name", NAMES)
def test_no_record_finds_its_node_already_connected(name):
    """hnsw.go:477-486 is out of a build's reach (the note in the kernel's `already connected` branch): 0 in every case"""
    links = hs.oracle_build(name)[3]
    assert np.count_nonzero(links["outcome"] == ALREADY) == 0


def test_chain_lengths():
    lengths = {}
    for name in NAMES:
        lengths[name] = {len(v) for v in hs.chains(hs.oracle_build(name)[3]).values()}
    for size in (63, 65, 129, 257):
        assert max(lengths[f"len-{size}"]) == size, lengths[f"len-{size}"]
    assert {1, 64, 128} <= lengths["len-257"]
    assert 256 in lengths["len-257"]
    assert max(lengths["chain-1000"]) >= 1000
    assert any(512 < n for n in lengths["chain-1000"])
    assert max(lengths["cube-m32"]) == 400 and max(lengths["cube-m16"]) == 400
    for name in ("hub-m8", "hub-m32", "hub-dot", "hub-cosine", "hub-ties-m32"):
        assert max(lengths[name]) == 300, (name, max(lengths[name]))
    assert max(lengths["hub-ties-m8"]) > 256


@pytest.mark.parametrize("name", ["hub-m8", "hub-m32", "hub-dot", "hub-cosine"])
def test_hub_work_at_the_edges_of_later_chunks(name):
    """the batch of rows 512..811: all 300 link back to row 0, so chain position = row - 512; the planted rows change the
    row at positions 64, 127, 128, 191 = lane 0 and lane 63 of chunks 1 and 2"""
    chain = _row0(name)[9]
    assert len(chain) == 300 and np.array_equal(chain["new_node"], 512 + np.arange(300))
    assert chain["deg"][0] == 2 * hs.case(name).m
    want = sorted(r - 512 for r in hs.HUB_WORK)
    assert want == [64, 127, 128, 191]
    changing = np.nonzero(_changes(chain))[0]
    assert set(want) <= set(changing.tolist())
    if name == "hub-cosine":
        return  # its row has tied members and settles only after the planted rows: see test_ties_*
    # ... and nothing else in the chain does: every other record is one the kernel may skip, among them a whole aligned
    # chunk (192..255) and the ragged tail (256..299) of a chain that is no multiple of 64
    assert changing.tolist() == want
    skip = _skippable(chain)
    assert np.array_equal(np.nonzero(~skip)[0], want)
    assert skip[192:256].all() and skip[256:300].all() and len(chain) % 64 != 0
    assert not _has(chain, TIE_MEMBERS).any()


@pytest.mark.parametrize("name", ["hub-m8", "hub-m32"])
def test_a_newcomer_as_far_as_the_last_member_is_not_skipped(name):
    """`cdist > last` in the chunk walk: a record whose distance EQUALS the last member's, on a fully chosen row without
    tied members, past the first chunk — and the reference's heap puts it in, so skipping it shows"""
    chain = _row0(name)[10]
    hit = np.nonzero(_has(chain, CHOSEN | TIE_LAST, none=TIE_MEMBERS | UNCHANGED | FARTHER))[0]
    assert hit.size == 1 and hit[0] >= 64, hit
    assert chain["new_node"][hit[0]] == 812 + 130
    rest = np.delete(np.arange(len(chain)), hit)
    assert _skippable(chain)[rest].all()


def test_ties_at_every_degree_level_and_metric():
    def tied(name, **where):
        links = hs.oracle_build(name)[3]
        sel = _has(links, TIE)
        for k, v in where.items():
            sel &= v(links[k])
        return int(np.count_nonzero(sel))

    assert tied("cube-m32", deg=lambda d: d == 64) >= 10000           # the 65-candidate heap
    assert tied("cube-m16", deg=lambda d: d == 32) >= 10000           # degree < 64
    assert tied("cube-m32", level=lambda l: l >= 1) >= 100
    assert tied("cube-m16", level=lambda l: l >= 1) >= 100
    assert tied("cube-dot") >= 10000 and hs.case("cube-dot").metric == o.METRIC_DOT
    assert tied("hub-cosine") >= 1000 and hs.case("hub-cosine").metric == o.METRIC_COSINE
    assert tied("hub-ties-m32", deg=lambda d: d == 64) >= 1000
    # every prune of the cube ties
    for name in ("cube-m16", "cube-m32", "cube-dot"):
        links = hs.oracle_build(name)[3]
        assert np.array_equal(_has(links, TIE), links["outcome"] == PRUNED)
    # negative distances under Dot with a hub: chains of 300 (test_chain_lengths), no ties needed
    c = hs.case("hub-dot")
    assert c.metric == o.METRIC_DOT and (c.base[1:] @ c.base[0] > 0).all()


def _stable_runs(name):
    """row 0's pruned records in build order: (skippable with tied members, changing)"""
    rows = _row0(name)
    ev = np.concatenate([rows[b] for b in sorted(rows)])
    return ev, _has(ev, CHOSEN | FARTHER | UNCHANGED | TIE_MEMBERS), _changes(ev)


@pytest.mark.parametrize("name,deg", [("hub-ties-m8", 16), ("hub-ties-m32", 64), ("hub-cosine", 16)])
def test_tied_rows_settle_change_and_settle_again(name, deg):
    """the `stable` seam: >= 100 records that find a fully chosen row with tied members, are strictly farther and leave it
    as it was; then a record that changes that row; then more of the first kind"""
    ev, settled, changing = _stable_runs(name)
    assert np.all(ev["deg"] == deg)
    first_change = next(i for i in np.nonzero(changing)[0] if settled[:i].sum() >= 100)
    assert settled[first_change:].sum() >= 100
    # a whole aligned chunk of them inside one chain
    assert any(_has(c, CHOSEN | FARTHER | UNCHANGED | TIE_MEMBERS)[64:128].all() for c in _row0(name).values() if len(c) >= 128)


def test_a_tied_row_that_never_settles():
    """hub-ties-m32's last two batches: a fully chosen row with tied members that strictly farther records CHANGE (the heap
    hands a tied pair back swapped), hundreds of times.  Whether they were applied shows in the debug totals of the GPU test;
    in the finished graph only if the swaps do not cancel, which is what swap-m8 and swap-m32 are for"""
    ev, settled, changing = _stable_runs("hub-ties-m32")
    unsettled = _has(ev, CHOSEN | FARTHER | TIE_MEMBERS, none=UNCHANGED)
    assert unsettled.sum() >= 200
    assert settled.sum() >= 500


@pytest.mark.parametrize("name", ["swap-m8", "swap-m32"])
def test_a_tied_pair_ends_the_build_swapped(name):
    """one tied pair in row 0, so a strictly farther record on the fully chosen row can change nothing but the order of the
    two: every such record that changes the row is one swap.  The build ends with an odd run of them, so a kernel that
    skipped that run would leave the pair the other way round (an even run would hide it)"""
    ev, settled, changing = _stable_runs(name)
    swaps = _has(ev, CHOSEN | FARTHER | TIE_MEMBERS, none=UNCHANGED)
    assert settled.sum() == 0 and swaps.sum() >= 500
    tail = len(ev) - 1 - int(np.nonzero(~swaps)[0].max())
    assert tail % 2 == 1 and tail >= 41, tail
    # the two are row 0's nearest members in the finished graph
    c = hs.case(name)
    pair = {1, 2}
    assert np.array_equal(c.base[1], -c.base[2]) and set(hs.oracle_build(name)[0][0, :2].tolist()) == pair


def test_a_row_fills_up_in_the_middle_of_a_chain():
    """ef = 1: every own row is its one candidate (appended rows everywhere), and row 0 goes from cnt < deg to full inside
    one chain: appends, then prunes"""
    found = 0
    for chain in hs.chains(hs.oracle_build("ef-1")[3]).values():
        out = chain["outcome"]
        k = int(np.count_nonzero(out == APPENDED))
        if 0 < k < len(out):
            assert np.all(out[:k] == APPENDED) and np.all(out[k:] == PRUNED)
            assert not (chain["flags"][k] & CHOSEN)  # appended, not chosen: the first prune takes the long way
            found += 1
    assert found >= 1


def test_ef_limits_reach_the_selection_seams():
    m = 8
    own = {ef: hs.oracle_build(f"ef-{ef}")[4] for ef in (1, 7, 8, 9, 16, 17, 1024)}
    for ef in own:
        assert hs.case(f"ef-{ef}").m == m and hs.case(f"ef-{ef}").ef == ef
    assert np.all(own[1]["candidates"] == 1)
    upper = lambda w: w[w["level"] >= 1]["candidates"]
    ground = lambda w: w[w["level"] == 0]["candidates"]
    assert own[7]["candidates"].max() == m - 1                              # <= m everywhere: selectNeighborsSimple only
    assert upper(own[8]).max() == m and np.count_nonzero(upper(own[8]) == m) >= 10
    assert upper(own[9]).max() == m + 1 and np.count_nonzero(upper(own[9]) == m + 1) >= 10
    assert ground(own[16]).max() == 2 * m and np.count_nonzero(ground(own[16]) == 2 * m) >= 100
    assert ground(own[17]).max() == 2 * m + 1 and np.count_nonzero(ground(own[17]) == 2 * m + 1) >= 100
    # kBuildMaxEf over fewer rows than ef: the lists are whatever the graph holds
    n = hs.case("ef-1024").base.shape[0]
    assert n < 1024 and 512 < ground(own[1024]).max() < 1024
    big = hs.oracle_build("ef-1024-n1400")[4]
    assert hs.case("ef-1024-n1400").base.shape[0] > 1024 and ground(big).max() == 1024
    assert np.count_nonzero(ground(big) == 1024) >= 100
