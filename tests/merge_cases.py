"""Chosen inputs for the fan-in merge (vg_merge_topk / _packed, vg_comm_all_gather_topk -> pack_keys_kernel, topk_merge_kernel,
merge_nan_replay_kernel in vecgo_amd/csrc/k_topk_merge.hip), the reference they are compared with, and a model of which of the
kernel's selection paths an input reaches.  Plain numpy; the reference is the oracle's CandidateHeap on the CPU.

Builders return (ids[lists, nq, k] uint32, scores[lists, nq, k] float32, id_offsets[lists] uint32).  Every list is best first,
unused slots hold 0xFFFFFFFF with +Inf (-Inf when descending), every query draws its own scores.  Local ids stay below SPAN
and list l's offset is l * SPAN, so (SegmentID, RowID) — what the engine's heap breaks ties by — orders like the global id."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

INVALID = 0xFFFFFFFF
KEY_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
SPAN = 100000          # local ids < SPAN; offsets are multiples of it (4097 lists stay below 2^32)
MERGE_BUF = 4096       # kMergeBuf
RANK_LIMIT = 1024      # `if (c <= 1024)`


# ---- the 64-bit selection key (vg_device.hpp f32_ordered / make_key) --------------------------------------------------------
def make_keys(ids, scores, descending, id_offsets=None):
    """keys[lists, ..., k] of (id, score) lists as pack_keys_kernel builds them; empty slots -> KEY_MAX"""
    ids = np.asarray(ids, np.uint32)
    u = np.asarray(scores, np.float32).view(np.uint32)
    s = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    if descending:
        s = ~s
    gid = ids.copy()
    if id_offsets is not None:
        off = np.asarray(id_offsets, np.uint32).reshape((-1,) + (1,) * (ids.ndim - 1))
        gid = (ids + off).astype(np.uint32)                       # wraps like the kernel's uint32 add
    keys = (s.astype(np.uint64) << np.uint64(32)) | gid.astype(np.uint64)
    return np.where(ids == INVALID, KEY_MAX, keys)


class MergePath(NamedTuple):
    path: str            # "rank" | "sort_one_trip" | "sort_multi_trip"
    survivors: int       # keys that pass the smaller bound (the kernel's counter, which may pass MERGE_BUF)
    head_bound: bool     # the k-th smallest list head was computed and is a real key
    tighter: str         # "kth" | "head" | "none": which bound is T
    trips: int           # sorts of the 4096-key buffer on the sort path, 0 on the rank path
    head_sort: int       # keys the head sort is padded to, 0 when it is skipped


def merge_path(ids, scores, k, descending, id_offsets=None) -> MergePath:
    """Which selection path topk_merge_kernel takes for ONE query: ids / scores are that query's [lists, k] slices.

    This is a MODEL OF THE CODE UNDER TEST, not a reference: it restates the kernel's own two bounds and its survivor count so
    that a test case can assert that it reaches the path it was written for.  It says nothing about what the merge should
    return (that is reference_merge below).  It mirrors vecgo_amd/csrc/k_topk_merge.hip, topk_merge_kernel:
      - first bound, the smallest k-th key of any list:            the loop `for (int l = tid; l < lists; ...) src[l * k + (k - 1)]`
      - second bound, the k-th smallest list head, computed only if `lists >= k && lists <= kMergeBuf && k >= 1`, over the
        heads padded to a power of two, and applied only if it is a real key (`hk != kKeyMax`)
      - survivors: every list walked from its head while `key != kKeyMax && key <= T` (the counter runs on past kMergeBuf)
      - `if (c <= 1024)` the brute-force rank, else the chunked sort: `take = min(total - pos, kMergeBuf - kept)`, `kept = k`
        after the first trip, until `pos >= total`.
    lists == 0 is merged as one empty list, as merge_topk_impl hands it over."""
    ids = np.asarray(ids, np.uint32).reshape(-1, k)
    scores = np.asarray(scores, np.float32).reshape(-1, k)
    keys = make_keys(ids, scores, descending, id_offsets)
    if keys.shape[0] == 0:
        keys = np.full((1, k), KEY_MAX, np.uint64)
    lists = keys.shape[0]
    t1 = keys[:, k - 1].min()
    hk = KEY_MAX
    head_sort = 0
    if lists >= k and lists <= MERGE_BUF and k >= 1:
        head_sort = 1
        while head_sort < lists:
            head_sort <<= 1
        hk = np.sort(keys[:, 0])[k - 1]
    head = bool(hk != KEY_MAX)
    T = min(t1, hk)
    tighter = "none" if T == KEY_MAX else ("head" if hk < t1 else "kth")
    ok = (keys != KEY_MAX) & (keys <= T)
    c = int(np.cumprod(ok, axis=1).sum())
    if c <= RANK_LIMIT:
        return MergePath("rank", c, head, tighter, 0, head_sort)
    total, pos, kept, trips = lists * k, 0, 0, 0
    while True:
        take = min(total - pos, MERGE_BUF - kept)
        pos += take
        kept = k
        trips += 1
        if pos >= total:
            break
    return MergePath("sort_one_trip" if trips == 1 else "sort_multi_trip", c, head, tighter, trips, head_sort)


# ---- builders -----------------------------------------------------------------------------------------------------------------
def _unique_scores(rng, n, descending):
    """n different float32 scores, best first; quarter steps around zero (exact in fp32), never a zero of either sign"""
    c = np.cumsum(rng.integers(1, 4, n)).astype(np.int64)
    v = ((c - c[n // 2] + 4 * rng.integers(-40, 40)) * 0.25 + 0.125).astype(np.float32)
    return v[::-1].copy() if descending else v


def _local_ids(rng, lists, nq, k):
    """different ids within every list, below SPAN, in no particular order"""
    x = np.cumsum(rng.integers(1, 50, (lists, nq, k)), axis=2)
    return rng.permuted(x, axis=2).astype(np.uint32)


def _empty(lists, nq, k, descending):
    return (np.full((lists, nq, k), INVALID, np.uint32),
            np.full((lists, nq, k), -np.inf if descending else np.inf, np.float32))


def offsets(lists):
    return (np.arange(lists, dtype=np.uint64) * SPAN).astype(np.uint32)


def round_robin(lists, k, nq, descending, seed):
    """the j-th best candidate overall goes to list j % lists: (k - 1) * lists + 1 keys survive the k-th-key bound"""
    rng = np.random.default_rng(seed)
    sc = np.empty((lists, nq, k), np.float32)
    for q in range(nq):
        sc[:, q, :] = _unique_scores(rng, lists * k, descending).reshape(k, lists).T
    return _local_ids(rng, lists, nq, k), sc, offsets(lists)


def blocked(lists, k, nq, descending, seed):
    """list l holds candidates l*k .. l*k + k-1 of the overall order (rows sorted by score): exactly k keys survive"""
    rng = np.random.default_rng(seed)
    sc = np.empty((lists, nq, k), np.float32)
    for q in range(nq):
        sc[:, q, :] = _unique_scores(rng, lists * k, descending).reshape(lists, k)
    return _local_ids(rng, lists, nq, k), sc, offsets(lists)


def tied(lists, k, nq, descending, seed, levels=4):
    """scores from `levels` integers: most of the order is decided by the global id, across lists"""
    rng = np.random.default_rng(seed)
    ids = _local_ids(rng, lists, nq, k)
    sc = rng.integers(0, levels, (lists, nq, k)).astype(np.float32)
    first = -sc if descending else sc
    order = np.lexsort((ids, first), axis=2)                       # best first within a list: (score, id)
    return np.take_along_axis(ids, order, 2), np.take_along_axis(sc, order, 2), offsets(lists)


def ragged(lengths, k, descending, seed):
    """lengths[lists, nq]: valid entries per list and query (0 .. k); the candidates are dealt to the lists at random"""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    lists, nq = lengths.shape
    assert lengths.min() >= 0 and lengths.max() <= k
    ids, sc = _empty(lists, nq, k, descending)
    local = _local_ids(rng, lists, nq, k)
    for q in range(nq):
        owner = rng.permutation(np.repeat(np.arange(lists), lengths[:, q]))
        v = _unique_scores(rng, owner.size, descending)           # best first, so every list's share is too
        for l in range(lists):
            n = int(lengths[l, q])
            sc[l, q, :n] = v[owner == l]
            ids[l, q, :n] = local[l, q, :n]
    return ids, sc, offsets(lists)


def shorter_than_k_lengths(lists, k, nq, seed):
    """every list shorter than k, an empty one and one of k - 1 among them"""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, k, (lists, nq))
    for q in range(nq):
        ln[q % lists, q] = 0
        ln[(q + 1) % lists, q] = k - 1
    return ln


def few_nonempty_lengths(lists, nq, per_list, seed):
    """len(per_list) non-empty lists per query, elsewhere nothing"""
    rng = np.random.default_rng(seed)
    ln = np.zeros((lists, nq), np.int64)
    for q in range(nq):
        ln[rng.permutation(lists)[:len(per_list)], q] = per_list
    return ln


# ---- the table ----------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    lists: int
    k: int
    layout: str                    # round_robin | blocked | tied | short | few | empty
    path: str
    survivors: Optional[int]       # None: per query (every valid key, asserted as such)
    head_bound: bool
    tighter: Optional[str] = None
    trips: int = 0
    head_sort: Optional[int] = None
    nq: int = 3


FEW = (1, 2, 3, 4, 2, 5, 1)        # 7 non-empty lists, 18 candidates < k = 20

TABLE = (
    Case("rr_5x16", 5, 16, "round_robin", "rank", 76, False, "kth"),
    Case("rr_31x34", 31, 34, "round_robin", "rank", 1024, False, "kth"),
    Case("rr_16x65", 16, 65, "round_robin", "sort_one_trip", 1025, False, "kth", 1),
    Case("rr_33x64", 33, 64, "round_robin", "sort_one_trip", 2080, False, "kth", 1),
    Case("rr_99x100", 99, 100, "round_robin", "sort_multi_trip", 9802, False, "kth", 3),
    Case("rr_5x1024", 5, 1024, "round_robin", "sort_multi_trip", 5116, False, "kth", 2),
    Case("rr_300x10", 300, 10, "round_robin", "rank", 10, True, "head", 0, 512),
    Case("blocked_300x10", 300, 10, "blocked", "rank", 10, True, "kth", 0, 512),
    Case("blocked_257x300", 257, 300, "blocked", "rank", 300, False, "kth", 0, 0),
    Case("rr_4097x2", 4097, 2, "round_robin", "sort_multi_trip", 4098, False, "kth", 3, 0),
    Case("blocked_4097x2", 4097, 2, "blocked", "rank", 2, False, "kth", 0, 0),
    Case("tied_40x64", 40, 64, "tied", "sort_one_trip", None, False, "kth", 1),
    Case("short_12x50", 12, 50, "short", "rank", None, False, "none"),
    Case("few_80x20", 80, 20, "few", "rank", None, False, "none", 0, 128),
    Case("one_1x1", 1, 1, "round_robin", "rank", 1, True, "kth", 0, 1),
    Case("none_0x8", 0, 8, "empty", "rank", 0, False, "none"),
)


def _readonly(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def build(case: Case, descending: bool):
    """the case's (ids, scores, id_offsets), built once and read-only"""
    seed = 1000 + 2 * TABLE.index(case) + int(descending) if case in TABLE else 7
    lists, k, nq = case.lists, case.k, case.nq
    if case.layout == "round_robin":
        r = round_robin(lists, k, nq, descending, seed)
    elif case.layout == "blocked":
        r = blocked(lists, k, nq, descending, seed)
    elif case.layout == "tied":
        r = tied(lists, k, nq, descending, seed)
    elif case.layout == "short":
        r = ragged(shorter_than_k_lengths(lists, k, nq, seed), k, descending, seed)
    elif case.layout == "few":
        r = ragged(few_nonempty_lengths(lists, nq, FEW, seed), k, descending, seed)
    elif case.layout == "empty":
        r = _empty(0, nq, k, descending) + (offsets(0),)
    else:
        raise ValueError(case.layout)
    return _readonly(*r)


def check_path(case: Case, ids, scores, off, descending):
    """every query of the case reaches the path the table states (asserts)"""
    for q in range(case.nq):
        m = merge_path(ids[:, q], scores[:, q], case.k, descending, off)
        valid = int(np.sum(ids[:, q] != INVALID))
        want = case.survivors if case.survivors is not None else valid
        if case.layout == "tied":
            want = m.survivors       # data-dependent; the path is what the case is for
            assert m.survivors > RANK_LIMIT
        assert (m.path, m.survivors, m.head_bound) == (case.path, want, case.head_bound), (case.name, q, m)
        assert m.trips == case.trips, (case.name, q, m)
        if case.tighter is not None:
            assert m.tighter == case.tighter, (case.name, q, m)
        if case.head_sort is not None:
            assert m.head_sort == case.head_sort, (case.name, q, m)


# ---- the reference --------------------------------------------------------------------------------------------------------------
def reference_merge(ids, scores, k, descending, id_offsets=None):
    """The engine's fan-in (engine/search.go:904-918) on the oracle's CandidateHeap: every list from its last valid entry to its
    first, push(score, l, id + off[l], k = k), then the pops, reversed.  Returns (ids[nq, k] uint32, scores[nq, k] float32,
    count[nq]); the slots past count hold 0xFFFFFFFF and +Inf / -Inf."""
    from oracle import oracle as o
    ids = np.asarray(ids, np.uint32)
    scores = np.asarray(scores, np.float32)
    lists, nq = ids.shape[0], ids.shape[1]
    off = np.zeros(lists, np.uint32) if id_offsets is None else np.asarray(id_offsets, np.uint32)
    gid = (ids + off[:, None, None]).astype(np.uint32)
    oid, osc = _empty(1, nq, k, descending)
    oid, osc = oid[0], osc[0]
    cnt = np.zeros(nq, np.int64)
    valid = (ids != INVALID).sum(axis=2)
    for q in range(nq):
        h = o.CandidateHeap(descending, cap=max(k, 4))
        for l in range(lists):
            n = int(valid[l, q])
            for s, g in zip(scores[l, q, :n][::-1].tolist(), gid[l, q, :n][::-1].tolist()):
                h.push(s, l, g, k=k)
        want = []
        while True:
            e = h.pop()
            if e is None:
                break
            want.append(e)
        h.close()
        want = want[::-1]
        cnt[q] = len(want)
        oid[q, :len(want)] = [e[2] for e in want]
        osc[q, :len(want)] = np.array([e[0] for e in want], np.float32)
    return oid, osc, cnt


@functools.lru_cache(maxsize=None)
def expected(case: Case, descending: bool):
    """reference_merge of the case, computed once and read-only"""
    ids, sc, off = build(case, descending)
    return _readonly(*reference_merge(ids, sc, case.k, descending, off))
