"""vg_bm25_update / _create_empty / _export on the device against tests/bm25_update_ref.py: after every update the exported image
equals the restatement's bit for bit, and a handful of queries answer as tests/bm25_ref.py's csr_search does over it and as a
fresh vg_bm25_create of the same arrays does (ids, float32 score bits, counts).  C = the update passes' posting chunk
(vg.BM25_UPDATE_CHUNK), T = the score kernel's doc tile, R = the radix passes' chunk of added postings."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import bm25_ref as ref
from tests import bm25_update_ref as uref
from tests import devbuf

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
UNSUPPORTED, INVALID_ARG = -5, -1
ROOT = Path(__file__).resolve().parents[1]
R = int(re.search(r"constexpr int kSortChunk = (\d+);", (ROOT / "vecgo_amd" / "csrc" / "k_bm25_update.hip").read_text()).group(1))


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def dev_u32(a):
    return devbuf.offset_like(np.asarray(a, np.uint32), 4)


def dev_i64(a):
    a = np.asarray(a, np.int64)
    flat = torch.empty(a.size + 1, dtype=torch.int64, device="cuda")
    view = flat[1:]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 != 0
    return view


class Room:
    """the bytes vg_bm25_stats reports, by the README's rule: both halves of the postings' and the offsets' ping-pong pairs and
    the per-doc arrays, each with its capacity; a buffer too small is replaced by max(need, 1.5 x the larger of the pair)"""

    def __init__(self, csr):
        self.post, self.alt_post, self.off, self.alt_off, self.docs = csr.post_doc.size, 0, csr.n_terms + 1, 0, csr.n_docs

    @staticmethod
    def _spare(alt, cur, need):
        if alt and alt >= need:
            return alt
        have = max(alt, cur)
        return max(need, have + have // 2, 1)

    def update(self, n_post_old, n_addp, n_terms_new, n_docs_new):
        alt_post = self._spare(self.alt_post, self.post, n_post_old + n_addp)
        alt_off = self._spare(self.alt_off, self.off, n_terms_new + 1)
        if n_docs_new > self.docs:
            self.docs = max(n_docs_new, self.docs + self.docs // 2)
        self.post, self.alt_post, self.off, self.alt_off = alt_post, self.post, alt_off, self.off

    def bytes(self, mapped):
        return (self.off + self.alt_off) * 8 + (self.post + self.alt_post) * 8 + self.docs * (8 if mapped else 4)


class Live:
    """a resident index and the restatement side by side"""

    def __init__(self, vg, ctx, csr=None, mapped=True):
        self.vg, self.ctx = vg, ctx
        if csr is None:
            self.csr = uref.Csr(mapped=mapped)
            self.bm = vg.Bm25.empty(ctx, with_doc_to_id=mapped)
            self.total_length, self.doc_count = 0, 0
        else:
            self.csr = csr
            self.total_length, self.doc_count = int(csr.doc_len.sum()), int((csr.doc_len > 0).sum())
            self.bm = vg.Bm25(ctx, *csr.arrays()[:4], self.total_length, self.doc_count, csr.doc_to_id)
        self.room = Room(self.csr)

    @staticmethod
    def arrays(adds):
        """adds: [(doc, length, id, {term: tf}), ...] -> add_docs, add_len, add_ids, add_off, add_terms, add_tf"""
        off, terms, tfs = [0], [], []
        for _, _, _, tf in adds:
            terms += list(tf)
            tfs += list(tf.values())
            off.append(len(terms))
        return (np.asarray([a[0] for a in adds], np.uint32), np.asarray([a[1] for a in adds], np.uint32), np.asarray([a[2] for a in adds], np.uint32),
                np.asarray(off, np.int64), np.asarray(terms, np.uint32), np.asarray(tfs, np.uint32))

    def call(self, del_docs, adds, n_docs, n_terms, total_length, doc_count, device=False, stream=None):
        docs, lens, ids, off, terms, tfs = adds if isinstance(adds, tuple) else self.arrays(adds)
        dels = np.asarray(del_docs, np.uint32)
        args = [dels, docs, lens, off, terms, tfs]
        if device:
            args = [dev_u32(dels), dev_u32(docs), dev_u32(lens), dev_i64(off), dev_u32(terms), dev_u32(tfs)]
        add_ids = None if not self.csr.mapped else (dev_u32(ids) if device else ids)
        self.bm.update(*args, n_docs, n_terms, total_length, doc_count, add_ids=add_ids, stream=stream)

    def update(self, del_docs=(), adds=(), n_docs=None, n_terms=None, totals=None, device=False, stream=None, queries=()):
        adds = adds if isinstance(adds, tuple) and len(adds) == 6 and isinstance(adds[0], np.ndarray) else self.arrays(list(adds))
        docs, lens, ids, off, terms, tfs = adds
        n_docs = self.csr.n_docs if n_docs is None else n_docs
        n_terms = self.csr.n_terms if n_terms is None else n_terms
        new = uref.update(self.csr, del_docs, docs, lens, off, terms, tfs, n_docs, n_terms, ids if self.csr.mapped else None)
        total_length, doc_count = totals or (int(new.doc_len.sum()), int((new.doc_len > 0).sum()))
        n_post_old = self.csr.post_doc.size
        self.call(del_docs, adds, n_docs, n_terms, total_length, doc_count, device, stream)
        if stream is not None:
            stream.synchronize()
        self.room.update(n_post_old, terms.size, n_terms, n_docs)
        self.csr, self.total_length, self.doc_count = new, total_length, doc_count
        self.check(queries)

    def same_image(self):
        got = self.bm.export()
        for name, g, w in zip(("term_off", "post_doc", "post_tf", "doc_len", "doc_to_id"), got, self.csr.arrays()):
            assert (g is None) == (w is None), name
            if g is not None:
                assert g.dtype == w.dtype and np.array_equal(g, w), (name, g[:16], w[:16])
        st = self.bm.stats()
        assert (st["docs"], st["terms"], st["postings"]) == (self.csr.n_docs, self.csr.n_terms, self.csr.post_doc.size)

    def idf(self, t):
        df = int(self.csr.term_off[t + 1] - self.csr.term_off[t]) if t < self.csr.n_terms else 0
        return ref.compute_idf(max(self.doc_count, 1), df)

    def check(self, queries=(), k=8, fresh=True):
        self.same_image()
        queries = [list(q) for q in queries]
        if not queries:
            return
        off = np.asarray(np.cumsum([0] + [len(q) for q in queries]), np.int32)
        terms = np.asarray([t for q in queries for t in q], np.uint32)
        idfs = np.asarray([self.idf(t) for t in terms], np.float64)
        ids, sc, cnt = self.bm.search(off, terms, idfs, k)
        if self.doc_count == 0:
            assert np.all(ids == INV) and np.all(np.isneginf(sc)) and np.all(cnt == 0)
            return
        c = self.csr
        for q in range(len(queries)):
            eid, esc, ecnt = ref.csr_search(c.term_off, c.post_doc, c.post_tf, c.doc_len, self.total_length, self.doc_count, terms[off[q]:off[q + 1]],
                                            idfs[off[q]:off[q + 1]], k, c.doc_to_id)
            assert cnt[q] == ecnt and np.array_equal(ids[q], eid) and np.array_equal(bits(sc[q]), bits(esc)), (q, ids[q], eid)
        if fresh:
            other = self.vg.Bm25(self.ctx, c.term_off, c.post_doc, c.post_tf, c.doc_len, self.total_length, self.doc_count, c.doc_to_id)
            fid, fsc, fcnt = other.search(off, terms, idfs, k)
            assert np.array_equal(fid, ids) and np.array_equal(bits(fsc), bits(sc)) and np.array_equal(fcnt, cnt)
            other.close()


def csr_from_lists(lists, n_docs, doc_len=None, ids=None):
    off, docs, tfs = [0], [], []
    for li in lists:
        docs += [d for d, _ in li]
        tfs += [c for _, c in li]
        off.append(len(docs))
    doc_len = np.full(n_docs, 7, np.uint32) if doc_len is None else doc_len
    return uref.Csr(off, docs, tfs, doc_len, np.arange(n_docs, dtype=np.uint32) + 100 if ids is None else ids)


@pytest.mark.parametrize("which", ["1", "C-1", "C", "C+1", "3C+5"])
def test_posting_seams(vg, ctx, which):
    C = vg.BM25_UPDATE_CHUNK
    L = {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "3C+5": 3 * C + 5}[which]
    n = L + 20
    rng = np.random.default_rng(L)
    # rare lists around the hot one in term_off: a chunk holds the hot list's end and the next lists' starts
    lists = [[(2, 1), (9, 2), (n - 1, 1)], [(5, 3)], [(d, 1 + d % 4) for d in range(L)], [(0, 2), (n - 2, 2)], [], [(1, 1), (3, 1), (4, 5), (n - 3, 1)]]
    live = Live(vg, ctx, csr_from_lists(lists, n, rng.integers(1, 30, n).astype(np.uint32)))
    total = live.csr.post_doc.size
    edge = {p for c in range(0, total + C, C) for p in (c - 1, c)} | set(range(C - 3, C + 4))   # chunks' first and last postings; a run over a seam
    dels = sorted({int(live.csr.post_doc[p]) for p in edge if 0 <= p < total} | {0, n - 2})      # ... and the whole of rare list 3
    adds = [(n, 4, 900, {2: 3, 6: 1}), (n + 1, 2, 901, {0: 1, 2: 1})]
    live.update(dels, adds, n_docs=n + 2, n_terms=8, queries=[[2], [0, 2, 5], [3], [6], [7, 1]])
    assert live.csr.term_off[4] == live.csr.term_off[3]         # list 3 is an empty range now, its id kept
    back = [(d, 3, 500 + d, {2: 2, 3: 1}) for d in dels[:3]]    # freed ids come back, into the list that was emptied too
    live.update([n], back, queries=[[2], [3, 2], [6]])


def test_merge_positions(vg, ctx):
    lists = [[(10, 1), (12, 2), (20, 3), (30, 1)], [(11, 1), (12, 1)], [(5, 2)], [(10, 4), (30, 4)]]
    live = Live(vg, ctx, csr_from_lists(lists, 32))
    adds = [(3, 5, 1, {0: 1, 7: 2}),            # below every doc of list 0 (a reused freed id); term 7 is new, 4 .. 6 stay unused
            (31, 5, 2, {0: 2, 3: 1}),           # above every doc of lists 0 and 3
            (15, 5, 3, {0: 3, 9: 1}),           # between two docs
            (13, 5, 4, {0: 4, 1: 1}),           # next to the deleted doc 12
            (6, 5, 5, {2: 9})]                  # in list 2, which the same call empties (doc 5 goes)
    live.update([12, 5], adds, n_docs=32, n_terms=10, queries=[[0], [1], [2], [7, 9], [4], [0, 3, 1]])
    assert live.csr.post_doc[live.csr.term_off[0]:live.csr.term_off[1]].tolist() == [3, 10, 13, 15, 20, 30, 31]
    assert np.diff(live.csr.term_off).tolist() == [7, 2, 1, 3, 0, 0, 0, 1, 0, 1]


def test_replace_ends_with_the_adds_length_and_id(vg, ctx):
    live = Live(vg, ctx, csr_from_lists([[(0, 1), (1, 1), (2, 1)], [(1, 2)]], 3))
    live.update([1, 1], [(1, 42, 777, {1: 5, 2: 1})], n_terms=3, queries=[[0], [1], [2]])   # (named twice in del_docs: fine)
    assert live.csr.doc_len[1] == 42 and live.csr.doc_to_id[1] == 777
    assert live.csr.post_doc.tolist() == [0, 2, 1, 1] and live.csr.post_tf.tolist() == [1, 1, 5, 1]
    live.update([2, 0, 1], [], queries=[[0], [1]])                                          # everything goes: doc_count == 0, empty answers
    assert live.doc_count == 0 and live.csr.post_doc.size == 0
    live.update([], [(2, 3, 5, {0: 1})], queries=[[0]])


def test_doc_tile_seam(vg, ctx):
    T = vg.BM25_TILE_DOCS
    rng = np.random.default_rng(2)
    some = sorted(rng.choice(T, size=200, replace=False).tolist())
    live = Live(vg, ctx, csr_from_lists([[(d, int(rng.integers(1, 5))) for d in some], [(T - 1, 2)]], T, rng.integers(1, 40, T).astype(np.uint32)))
    live.update([], [(T, 3, 4242, {0: 9, 1: 1})], n_docs=T + 1, queries=[[0], [1], [1, 0]], )
    ids, _, cnt = live.bm.search(np.asarray([0, 1], np.int32), np.asarray([1], np.uint32), np.asarray([live.idf(1)]), 4)
    assert cnt[0] == 2 and 4242 in ids[0].tolist()              # the doc of the second tile is found


def batch_of(rng, n_post, n_terms, doc0, n_docs_span):
    """docs doc0 .. with 1 .. 5 distinct random terms each, n_post postings in all"""
    adds, left = [], n_post
    docs = rng.permutation(n_docs_span)[:n_post] + doc0           # in no order
    while left:
        c = min(left, int(rng.integers(1, 6)), n_terms)
        terms = rng.choice(n_terms, size=c, replace=False)
        adds.append((int(docs[len(adds)]), int(rng.integers(1, 50)), 7000 + len(adds), {int(t): int(rng.integers(1, 9)) for t in terms}))
        left -= c
    return adds


@pytest.mark.parametrize("which", ["1", "R-1", "R", "R+1", "2R+7"])
def test_added_batch_sizes_around_the_radix_chunk(vg, ctx, which):
    """(the ordering pass has one form, the radix sort: its seam is the chunk of one workgroup)  12 terms and fewer than 2^16 docs:
    the sort runs three of its eight digits"""
    n_post = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+7": 2 * R + 7}[which]
    rng = np.random.default_rng(n_post)
    live = Live(vg, ctx, csr_from_lists([[(d, 1) for d in range(0, 300, 3)], [(7, 2), (8, 2)]], 300))
    adds = batch_of(rng, n_post, 12, 300, 3 * R)
    live.update([6, 7], adds, n_docs=300 + 3 * R, n_terms=12, queries=[[0], [1], [11, 3], [5]])


def test_a_batch_whose_ids_need_every_radix_digit(vg, ctx):
    """docs and terms beyond 2^24: no digit of (term << 32 | doc) is constant"""
    big = (1 << 24) + 2
    rng = np.random.default_rng(9)
    docs = np.unique(np.concatenate([rng.integers(0, big, 120), [0, big - 1, 1 << 24, 255, 256, 65536]]))
    adds = []
    for d in rng.permutation(docs):
        terms = np.unique(np.concatenate([rng.integers(0, big, 2), [big - 1] if d % 3 == 0 else [5]]))
        adds.append((int(d), 4, 0, {int(t): int(rng.integers(1, 5)) for t in terms}))
    live = Live(vg, ctx, mapped=False)
    live.update([], adds, n_docs=big, n_terms=big)
    live.check([[big - 1], [5], [5, big - 1]], fresh=False)      # (a fresh index of 2^24 terms is a 134 MB upload: the image was compared)
    live.update([int(docs[0])], [(3, 2, 0, {big - 1: 1, 0: 1})])
    live.check([[big - 1], [0]], fresh=False)


def test_from_empty_follows_the_memory_index(vg, ctx):
    live = Live(vg, ctx, mapped=True)
    ids, sc, cnt = live.bm.search(np.asarray([0, 1, 1], np.int32), np.asarray([0], np.uint32), np.asarray([1.0]), 3)
    assert np.all(ids == INV) and np.all(np.isneginf(sc)) and cnt.tolist() == [0, 0]
    drv = uref.Driver()
    emptied = 0
    for batch in uref.zipf_script(1, 400):
        for op in batch:
            drv.add(op[1], op[2]) if op[0] == "add" else drv.delete(op[1])
        a = drv.flush()
        live.update(a["del_docs"], (a["add_docs"], a["add_len"], a["add_ids"], a["add_off"], a["add_terms"], a["add_tf"]), n_docs=a["n_docs"],
                    n_terms=a["n_terms"], totals=(a["total_length"], a["doc_count"]))
        assert drv.lists_equal(uref.Csr(*live.bm.export()))
        emptied += a["doc_count"] == 0
        texts = ["w0", "w1 w3", "w0 w2 w5 w9", "w39 w17", "nothing"]
        q = [drv.query(t) for t in texts]
        off = np.asarray(np.cumsum([0] + [len(t) for t, _ in q]), np.int32)
        ids, sc, cnt = live.bm.search(off, np.asarray([t for ts, _ in q for t in ts], np.uint32), np.asarray([w for _, ws in q for w in ws], np.float64), 7)
        for i, text in enumerate(texts):
            want = drv.mem.search(text, 7, sort=True)
            assert cnt[i] == len(want) and ids[i, :cnt[i]].tolist() == [pk for pk, _ in want], (text, ids[i], want)
            assert np.array_equal(bits(sc[i, :cnt[i]]), bits([s for _, s in want])), text
    assert emptied == 1 and drv.mem.doc_count > 0


def test_capacity_and_the_bytes_held(vg, ctx):
    rng = np.random.default_rng(5)
    live = Live(vg, ctx, csr_from_lists([[(d, 1) for d in range(100)], [(d, 2) for d in range(0, 100, 2)]], 100))
    assert live.bm.stats()["bytes"] == live.room.bytes(True) == 3 * 8 + 150 * 8 + 100 * 8
    live.update([], batch_of(rng, 400, 6, 100, 500), n_docs=600, n_terms=6, queries=[[0], [5]])   # 150 -> 550 postings: beyond 1.5 x
    assert live.bm.stats()["bytes"] == live.room.bytes(True)
    assert live.room.post == 550 and live.room.alt_post == 150 and live.room.docs == 600
    live.update(list(range(1, 600)), [], queries=[[0], [1]])                                        # nearly all of them go
    assert live.csr.post_doc.size == 2 and live.bm.stats()["bytes"] == live.room.bytes(True)
    assert live.room.post == 825                                                                    # 550 did not fit 150: 1.5 x 550
    live.update([], [(9, 3, 1, {0: 1, 4: 2})], queries=[[0], [4]])
    assert live.bm.stats()["bytes"] == live.room.bytes(True) and (live.room.post, live.room.alt_post) == (550, 825)


@pytest.mark.parametrize("device", [False, True])
def test_an_add_into_a_live_slot_fails_and_changes_nothing(vg, ctx, device):
    live = Live(vg, ctx, csr_from_lists([[(0, 1), (4, 1), (9, 2)], [(4, 3)]], 10))
    queries = [[0], [1], [0, 1]]
    off, terms = np.asarray([0, 1, 2, 4], np.int32), np.asarray([0, 1, 0, 1], np.uint32)
    idfs = np.asarray([live.idf(t) for t in terms])
    before = live.bm.search(off, terms, idfs, 5)
    bytes_before = None
    for attempt in range(2):                                    # (the second attempt finds the spare buffers of the first)
        with pytest.raises(vg.VecgoHipError) as e:
            live.call([9], [(4, 2, 5, {1: 1, 2: 1}), (9, 2, 6, {0: 1})], 10, 3, 20, 3, device=device)   # doc 4 lives in list 1; 9 is a replace
        assert e.value.status == INVALID_ARG and "doc 4 " in e.value.message
        live.check(queries)                                     # the image, the sizes and the answers are the old ones
        after = live.bm.search(off, terms, idfs, 5)
        assert all(np.array_equal(devbuf.raw(x), devbuf.raw(y)) for x, y in zip(before, after))
        bytes_before = bytes_before or live.bm.stats()["bytes"]
        assert live.bm.stats()["bytes"] == bytes_before
    live.room.alt_post, live.room.alt_off = 7, 4                # (the failed calls left their spare buffers: 4 + 3 postings, 3 + 1 offsets)
    assert live.bm.stats()["bytes"] == live.room.bytes(True)
    live.update([9, 4], [(4, 2, 5, {1: 1, 2: 1}), (9, 2, 6, {0: 1})], n_terms=3, device=device, queries=queries + [[2]])


def test_refusals_name_the_number(vg, ctx):
    live = Live(vg, ctx, csr_from_lists([[(0, 1), (1, 1)]], 5))
    ident = Live(vg, ctx, uref.Csr([0, 1], [0], [1], [1, 0], None))

    def refused(lv, status, text, *args, **kw):
        with pytest.raises(vg.VecgoHipError) as e:
            lv.bm.update(*args, **kw)
        assert e.value.status == status and text in e.value.message, e.value.message
        lv.check([[0]])
    none, one = np.zeros(0, np.uint32), np.ones(1, np.uint32)
    refused(live, INVALID_ARG, "n_docs_new = 4", none, none, none, None, none, none, 4, 1, 2, 2)
    refused(live, INVALID_ARG, "n_terms_new = 0", none, none, none, None, none, none, 5, 0, 2, 2)
    refused(live, UNSUPPORTED, str(1 << 31), none, none, none, None, none, none, 1 << 31, 1, 2, 2)
    refused(live, UNSUPPORTED, str((1 << 32) - 1), none, none, none, None, none, none, 5, (1 << 32) - 1, 2, 2)
    refused(live, INVALID_ARG, "add_ids is required", none, [2], one, [0, 1], [0], one, 5, 1, 3, 3)
    refused(ident, INVALID_ARG, "add_ids", none, [1], one, [0, 1], [0], one, 2, 1, 2, 2, add_ids=one)
    refused(live, INVALID_ARG, "doc 3 twice", none, [3, 3], [1, 1], [0, 1, 2], [0, 0], [1, 1], 5, 1, 4, 4, add_ids=[1, 2])
    refused(live, INVALID_ARG, "term 0 twice", none, [3], one, [0, 2], [0, 0], [1, 1], 5, 1, 3, 3, add_ids=one)
    refused(live, INVALID_ARG, "term 6", none, [3], one, [0, 1], [6], one, 5, 2, 3, 3, add_ids=one)
    refused(live, INVALID_ARG, "doc 5", none, [5], one, [0, 1], [0], one, 5, 1, 3, 3, add_ids=one)
    refused(live, INVALID_ARG, "doc 7", [7], none, none, None, none, none, 9, 1, 2, 2)
    refused(live, INVALID_ARG, "add_off decreases at added doc 1", none, [2, 3], [1, 1], [0, 1, 0], [0], one, 5, 1, 3, 3, add_ids=[1, 2])
    with pytest.raises(vg.VecgoHipError) as e:                   # vg_bm25_create keeps refusing an index without docs
        vg.Bm25(ctx, np.asarray([0, 1], np.int64), np.zeros(1, np.uint32), np.ones(1, np.uint32), np.ones(1, np.uint32), 1, 0)
    assert e.value.status == INVALID_ARG and "doc_count = 0" in e.value.message
    ident.update([], [(1, 2, 0, {0: 1})], queries=[[0]])          # an identity index takes updates without ids
    ident.update([], [], queries=[[0]])                           # nothing to do: served
    ident.update([], [], n_docs=4, n_terms=3, totals=(9, 3), queries=[[0], [2]])   # only the sizes and the constants change


def test_device_buffers_at_odd_offsets_on_a_callers_stream(vg, ctx):
    C = vg.BM25_UPDATE_CHUNK
    rng = np.random.default_rng(12)
    n = C + 50
    live = Live(vg, ctx, csr_from_lists([[(d, 1 + d % 3) for d in range(n)], [(d, 2) for d in range(0, n, 5)]], n,
                                         rng.integers(1, 30, n).astype(np.uint32)))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        live.update(list(range(0, n, 7)), batch_of(rng, 700, 5, n, 900), n_docs=n + 900, n_terms=5, device=True, stream=stream,
                    queries=[[0], [1, 4], [3]])
        live.update([3, 4, n + 5], [(3, 8, 1234, {0: 2, 4: 1})], device=True, stream=stream, queries=[[0], [4]])


def test_replayed_keeps_counting_across_an_update(vg, ctx):
    live = Live(vg, ctx, csr_from_lists([[(d, 1) for d in range(6)]], 6))   # six identical docs: a query for k = 3 ties
    off, terms, idfs = np.asarray([0, 1], np.int32), np.asarray([0], np.uint32), np.asarray([live.idf(0)])
    live.bm.search(off, terms, idfs, 3)
    assert live.bm.replayed() == 1
    live.update([0], [(6, 7, 106, {0: 1})], n_docs=7)
    assert live.bm.replayed() == 1
    live.bm.search(off, terms, np.asarray([live.idf(0)]), 3)
    assert live.bm.replayed() == 2
