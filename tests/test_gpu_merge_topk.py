"""The fan-in merge (vg_merge_topk, vg_merge_topk_packed, vg_comm_all_gather_topk: pack_keys_kernel -> topk_merge_kernel ->
merge_nan_replay_kernel) on every selection path of topk_merge_kernel: the brute-force rank, the one-trip and the multi-trip
sort, the survivor counter past its buffer, the head bound with its power-of-two padding and where it is skipped — each case
asserts, by tests/merge_cases.merge_path, that it reaches the path it was written for.  The reference is the engine's fan-in on
the oracle's CandidateHeap (merge_cases.reference_merge); the kernels only sort and copy, so ids and score bits are compared
exactly (NaN == NaN where a list holds one).  Also pinned here: a candidate that repeats across lists is kept twice, adjacent,
and zero scores of opposite sign tie as floats (the lower global id first), as InternalCandidateBetter has it."""
import numpy as np
import pytest

from tests import merge_cases as mc

pytestmark = pytest.mark.gpu

INVALID = mc.INVALID
SENTINEL = 0x7EADBEEF          # an id no case produces; output buffers are pre-filled with it where a slot could stay unwritten
VG_ERR_UNSUPPORTED = -5


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same_scores(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def host(t):
    """(ids uint32, scores float32) on the host from numpy arrays or torch tensors"""
    i, s = t
    if not isinstance(i, np.ndarray):
        i, s = i.cpu().numpy(), s.cpu().numpy()
    return np.asarray(i).view(np.uint32), np.asarray(s, np.float32)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def packed_image(ids, sc):
    """[lists][2][nq][k]: [l][0] the ids of list l, [l][1] the bit patterns of its scores (device tensor)"""
    return to_dev(np.stack([ids.view(np.int32), sc.view(np.int32)], axis=1))


def sentinel_out(nq, k):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.full((nq, k), SENTINEL, dtype=torch.int32, device=dev), torch.full((nq, k), 12345.0, dtype=torch.float32, device=dev))


def check_against(got, want, descending, nan_ok=False):
    gi, gs = host(got)
    wi, ws, cnt = want
    nq, k = wi.shape
    assert gi.shape == (nq, k) and gs.shape == (nq, k)
    pad = np.float32(-np.inf if descending else np.inf)
    for q in range(nq):
        r = int(cnt[q])
        assert np.array_equal(gi[q, :r], wi[q, :r]), (q, r, np.flatnonzero(gi[q, :r] != wi[q, :r])[:8], gi[q, :r][:12], wi[q, :r][:12])
        if nan_ok:
            assert same_scores(gs[q, :r], ws[q, :r]), (q, gs[q, :r][:12], ws[q, :r][:12])
        else:
            assert np.array_equal(bits(gs[q, :r]), bits(ws[q, :r])), (q, gs[q, :r][:12], ws[q, :r][:12])
        assert np.all(gi[q, r:] == INVALID), (q, r, gi[q, r:][:12])
        assert np.all(bits(gs[q, r:]) == bits(pad)), (q, r, gs[q, r:][:12])


def dense_and_packed(vg, ctx, ids, sc, k, metric, off, want, nan_ok=False, prefill=False):
    """merge_topk on host arrays against `want`, then merge_topk_packed on the device image: bit for bit the dense result"""
    from vecgo_amd import api
    desc = metric != 0
    lists, nq = ids.shape[0], ids.shape[1]
    dense = api.merge_topk(ctx, ids, sc, k, metric=metric, id_offsets=off, out=sentinel_out(nq, k) if prefill else None)
    check_against(dense, want, desc, nan_ok)
    got = api.merge_topk_packed(ctx, packed_image(ids, sc), lists, nq, k, metric=metric,
                                id_offsets=None if off is None else to_dev(off), out=sentinel_out(nq, k) if prefill else None)
    di, ds = host(dense)
    pi, ps = host(got)
    assert np.array_equal(pi, di)
    assert np.array_equal(bits(ps), bits(ds))
    return di, ds


# ---- the table: every selection path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("case", mc.TABLE, ids=lambda c: c.name)
def test_merge_on_every_selection_path(vg, ctx, case, metric):
    desc = metric != 0
    ids, sc, off = mc.build(case, desc)
    mc.check_path(case, ids, sc, off, desc)
    dense_and_packed(vg, ctx, ids, sc, case.k, metric, off if case.lists else None, mc.expected(case, desc))


# ---- limits -------------------------------------------------------------------------------------------------------------------
def test_limits(vg, ctx):
    from vecgo_amd import api
    ids, sc, off = mc.round_robin(2, 1025, 1, False, 5)
    with pytest.raises(vg.VecgoHipError) as e:
        api.merge_topk(ctx, ids, sc, 1025, metric=0, id_offsets=off)
    assert e.value.status == VG_ERR_UNSUPPORTED
    ids, sc, off = mc.round_robin(2, 1024, 1, False, 5)      # the documented limit itself is served
    gi, gs = api.merge_topk(ctx, ids, sc, 1024, metric=0, id_offsets=off)
    check_against((gi, gs), mc.reference_merge(ids, sc, 1024, False, off), False)
    with pytest.raises(vg.VecgoHipError) as e:
        api.merge_topk(ctx, ids[:, :, :8].copy(), sc[:, :, :8].copy(), 8, metric=3, id_offsets=off)
    assert e.value.status == VG_ERR_UNSUPPORTED


@pytest.mark.parametrize("nq,k", [(0, 8), (4, 0)])
def test_nothing_to_merge_leaves_the_outputs_alone(vg, ctx, nq, k):
    from vecgo_amd import api
    ids = np.zeros((3, nq, k), np.uint32)
    sc = np.zeros((3, nq, k), np.float32)
    for out in ((np.full(16, SENTINEL, np.uint32), np.full(16, 12345.0, np.float32)), sentinel_out(4, 4)):
        api.merge_topk(ctx, ids, sc, k, metric=0, id_offsets=mc.offsets(3), out=out)
        api.merge_topk_packed(ctx, packed_image(ids, sc), 3, nq, k, metric=2, out=out)
        oi, os_ = host(out)
        assert np.all(oi == SENTINEL) and np.all(os_ == np.float32(12345.0))


# ---- device tensors in, device tensors out ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("name", ["rr_31x34", "rr_99x100"])
def test_device_tensors_equal_host_arrays(vg, ctx, name, metric):
    """a rank case and a multi-trip case with every buffer a torch device tensor"""
    import torch
    from vecgo_amd import api
    case = next(c for c in mc.TABLE if c.name == name)
    desc = metric != 0
    ids, sc, off = mc.build(case, desc)
    want = api.merge_topk(ctx, ids, sc, case.k, metric=metric, id_offsets=off)
    got = api.merge_topk(ctx, to_dev(ids), to_dev(sc), case.k, metric=metric, id_offsets=to_dev(off))
    assert isinstance(got[0], torch.Tensor) and got[0].is_cuda and got[1].is_cuda
    gi, gs = host(got)
    assert np.array_equal(gi, want[0]) and np.array_equal(bits(gs), bits(want[1]))
    check_against(got, mc.expected(case, desc), desc)


def test_all_gather_topk_with_a_world_of_one(vg, ctx):
    from vecgo_amd import api
    import torch.distributed  # noqa: F401  (torch maps its own librccl when RCCL is first used; the library reuses a mapped one)
    nq, k = 5, 200
    off = np.array([7], np.uint32)
    comm = api.Comm(ctx, 1, 0, api.Comm.unique_id())
    try:
        for metric in (0, 2):
            desc = metric != 0
            ids, sc, _ = mc.round_robin(1, k, nq, desc, 11 + metric)
            out = comm.all_gather_topk(to_dev(ids[0]), to_dev(sc[0]), k, metric=metric, id_offsets=to_dev(off))
            want = api.merge_topk(ctx, ids, sc, k, metric=metric, id_offsets=off)
            gi, gs = host(out)
            assert np.array_equal(gi, want[0]) and np.array_equal(bits(gs), bits(want[1]))
            check_against(out, mc.reference_merge(ids, sc, k, desc, off), desc)
    finally:
        comm.close()


# ---- NaN replay beyond one ballot -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("lists,k", [(3, 200), (2, 1024)])
def test_nan_replay_beyond_one_ballot(vg, ctx, lists, k, metric):
    """k > 64: the ballot loop that counts a list's valid prefix runs 4 resp. 16 times.  Query 0 has no NaN and keeps the key
    merge's answer; 1: a NaN at the head of a list; 2: at the tail; 3: in the middle; 4: an all-NaN list; 5: a NaN in a ragged
    list of valid length 130 = two full ballots and a partial one.  (The lists stay best first where no NaN is involved.)"""
    desc = metric != 0
    nq = 6
    ln = np.full((lists, nq), k, np.int64)
    ln[0, 5] = 130
    ids, sc, off = mc.ragged(ln, k, desc, 300 + lists + metric)
    # list 0 is pushed first, while the heap fills, so its NaNs enter (one at the tail becomes the root and turns everything
    # after the k-th push away); a NaN of a later list meets a full heap and is turned away itself
    sc[0, 1, 0] = np.nan
    sc[0, 2, k - 1] = np.nan
    sc[0, 3, k // 2 + 1] = np.nan; sc[lists - 1, 3, k // 3] = np.nan
    sc[0, 4, :] = np.nan
    sc[0, 5, 77] = np.nan
    assert int(np.sum(ids[0, 5] != INVALID)) == 130 and not np.isnan(sc[:, 0]).any()
    want = mc.reference_merge(ids, sc, k, desc, off)
    assert np.isnan(want[1][1:]).any(axis=1).all() and np.isnan(want[1][4]).all()   # the heap's layout decides these queries
    di, ds = dense_and_packed(vg, ctx, ids, sc, k, metric, off, want, nan_ok=True)
    # query 0 is the plain order by (score, global id)
    v = ids[:, 0] != INVALID
    g = (ids[:, 0] + off[:, None])[v]
    s = sc[:, 0][v]
    order = np.lexsort((g, -s if desc else s))[:k]
    assert np.array_equal(di[0], g[order]) and np.array_equal(bits(ds[0]), bits(s[order]))


# ---- a candidate that repeats across lists ----------------------------------------------------------------------------------------
def _with_duplicates(lists, k, nq, desc, seed, through_offsets):
    """round-robin lists in which, per query, three candidates of list 0 appear again in another list at the same place of the
    order (same score, same global id): places 1 and 2 of the merged order, k/2 and k/2 + 1, and k - 1 and k (one copy in the result, one cut).  through_offsets:
    the copy's local id differs and the lists' offsets make the global ids coincide; else id_offsets = None and the local ids
    are the global ones."""
    ids, sc, _ = mc.round_robin(lists, k, nq, desc, seed)
    # ids different across ALL lists of a query, so that the planted copies are the only repeats
    rng = np.random.default_rng(seed + 1)
    for q in range(nq):
        ids[:, q, :] = (rng.permutation(lists * k) + 1000).reshape(lists, k)
    off = None
    if through_offsets:
        off = (np.arange(lists, dtype=np.uint32) * np.uint32(7)).astype(np.uint32)   # small: global ids of different lists can meet
        ids = ids * np.uint32(7 * lists)                                             # ... but only where planted
    # candidate j of the overall order sits in list j % lists at place j // lists; its copy replaces candidate j + 1 (in the
    # next list), so both lists stay best first and the copies take places j and j + 1 of the merged order
    for j in (1, k // 2, k - 1):
        (ls, ps), (ld, pd) = (j % lists, j // lists), ((j + 1) % lists, (j + 1) // lists)
        sc[ld, :, pd] = sc[ls, :, ps]
        shift = int(off[ls]) - int(off[ld]) if through_offsets else 0
        ids[ld, :, pd] = (ids[ls, :, ps].astype(np.int64) + shift).astype(np.uint32)
    return ids, sc, off


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("through_offsets", [False, True], ids=["no_offsets", "offsets_collide"])
@pytest.mark.parametrize("lists,k,path", [(5, 16, "rank"), (33, 64, "sort_one_trip")])
def test_a_candidate_listed_twice_is_kept_twice(vg, ctx, lists, k, path, through_offsets, metric):
    """The same (score, global id) in two lists — replicated or overlapping shards — comes out as the engine's heap has it
    (its candidates differ in SegmentID): both copies, adjacent, and every slot up to the result count written.  The output
    buffers are pre-filled with a sentinel id, so a slot the kernel skips is seen."""
    desc = metric != 0
    nq = 3
    ids, sc, off = _with_duplicates(lists, k, nq, desc, 500 + lists + metric, through_offsets)
    keys = mc.make_keys(ids, sc, desc, off)
    assert np.all(keys[:, :, 1:] >= keys[:, :, :-1])                          # the lists are best first
    for q in range(nq):
        assert keys[:, q].size - np.unique(keys[:, q]).size == 3              # three repeats, nothing else
        assert mc.merge_path(ids[:, q], sc[:, q], k, desc, off).path == path
    want = mc.reference_merge(ids, sc, k, desc, off)
    wi = want[0]
    for q in range(nq):                                                       # the reference keeps both copies, adjacent
        rep = np.flatnonzero(wi[q, 1:] == wi[q, :-1])
        assert rep.size >= 2 and np.all(want[2] == k)
    di, _ = dense_and_packed(vg, ctx, ids, sc, k, metric, off, want, prefill=True)
    assert not np.any(di == SENTINEL)


# ---- zero scores of opposite sign ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 2])
def test_zeros_of_opposite_sign_tie(vg, ctx, metric):
    """-0.0 == +0.0 for InternalCandidateBetter, so among zero scores the lower (segment, row) = the lower global id wins; the
    64-bit key orders -0.0 strictly before +0.0 (after it when descending).  Lists whose zeros have ONE sign each (so every list
    is best first either way), the sign that the key prefers in the HIGHER lists: which zeros make the cut at k and their order
    differ between the two orders.  Scores come back with the sign they were given.  The last query has zeros of one sign only."""
    desc = metric != 0
    lists, k, nq = 4, 8, 4
    rng = np.random.default_rng(700 + metric)
    ids, sc, off = mc.ragged(np.full((lists, nq), k), k, desc, 710 + metric)
    key_first = np.float32(0.0) if desc else np.float32(-0.0)       # the sign the key order puts first
    key_last = np.float32(-0.0) if desc else np.float32(0.0)
    for q in range(nq):
        for l in range(lists):
            zero = key_last if (l < 2) != (q == 1) else key_first      # query 1: the key's favourites in the LOWER lists
            if q == nq - 1:
                zero = key_last
            better = (rng.integers(1, 40) * 0.5)                       # one candidate better than any zero, three zeros,
            worse = np.sort(rng.permutation(40)[:k - 4] + 1) * 0.5 + 100    # the rest worse
            row = np.concatenate([[-better], [0.0] * 3, worse]).astype(np.float32)
            sc[l, q] = -row if desc else row
            sc[l, q, 1:4] = zero
            ids[l, q, :] = np.sort(ids[l, q, :])                       # ties inside a list: ascending id
    assert np.signbit(sc[sc == 0]).any() and not np.signbit(sc[sc == 0]).all()
    want = mc.reference_merge(ids, sc, k, desc, off)
    # key order and float order disagree on queries 0 and 2 (and only there: 1 has the key's favourites in the lower lists)
    keys = mc.make_keys(ids, sc, desc, off)
    for q in range(nq):
        by_key = np.sort(keys[:, q].ravel())[:k] & np.uint64(0xFFFFFFFF)
        assert np.array_equal(by_key.astype(np.uint32), want[0][q]) == (q in (1, 3)), q
    dense_and_packed(vg, ctx, ids, sc, k, metric, off, want)
