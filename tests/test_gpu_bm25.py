"""vg_bm25_search on the device against tests/bm25_ref.py (lexical/bm25 MemoryIndex.Search restated): ids, float32 score bits
and counts are equal, exactly.  The idf doubles are computed once on the host and handed to both sides.  T = the score
kernel's doc tile (vg.BM25_TILE_DOCS)."""
import itertools

import numpy as np
import pytest
import torch

from tests import bm25_ref as ref
from tests import devbuf, hooks

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
UNSUPPORTED, INVALID_ARG = -5, -1


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


class Corpus:
    """CSR postings from {term: [(doc, tf), ...]} (ascending docs), the resident index and the reference over the same arrays"""

    def __init__(self, vg, ctx, n_docs, lists, doc_len, total_length=None, doc_count=None, doc_to_id=None):
        off, docs, tfs = [0], [], []
        for li in lists:
            docs += [d for d, _ in li]
            tfs += [c for _, c in li]
            off.append(len(docs))
        self.term_off = np.asarray(off, np.int64)
        self.post_doc = np.asarray(docs, np.uint32)
        self.post_tf = np.asarray(tfs, np.uint32)
        self.doc_len = np.asarray(doc_len, np.uint32)
        assert self.doc_len.size == n_docs
        self.total_length = int(self.doc_len.sum()) if total_length is None else total_length
        self.doc_count = max(int((self.doc_len > 0).sum()), 1) if doc_count is None else doc_count
        self.doc_to_id = None if doc_to_id is None else np.asarray(doc_to_id, np.uint32)
        self.df = np.diff(self.term_off)
        self.bm = vg.Bm25(ctx, self.term_off, self.post_doc, self.post_tf, self.doc_len, self.total_length, self.doc_count, self.doc_to_id)

    def idf(self, t):
        return ref.compute_idf(self.doc_count, int(self.df[t])) if t < self.df.size else 1.0

    def arrays(self, queries):
        """queries: [[term, ...] | [(term, idf), ...], ...] -> (q_term_off, q_terms, q_idf)"""
        off, terms, idfs = [0], [], []
        for q in queries:
            for t in q:
                t, w = t if isinstance(t, tuple) else (t, self.idf(t))
                terms.append(t)
                idfs.append(w)
            off.append(len(terms))
        return np.asarray(off, np.int32), np.asarray(terms, np.uint32), np.asarray(idfs, np.float64)

    def expect(self, terms, idfs, k):
        return ref.csr_search(self.term_off, self.post_doc, self.post_tf, self.doc_len, self.total_length, self.doc_count, terms, idfs, k,
                              self.doc_to_id)

    def check(self, queries, k, run=None):
        off, terms, idfs = self.arrays(queries)
        ids, sc, cnt = (run or (lambda o, t, w: self.bm.search(o, t, w, k)))(off, terms, idfs)
        ids, sc, cnt = devbuf.to_host(ids).view(np.uint32), devbuf.to_host(sc), devbuf.to_host(cnt)
        for q in range(len(queries)):
            eid, esc, ecnt = self.expect(terms[off[q]:off[q + 1]], idfs[off[q]:off[q + 1]], k)
            assert cnt[q] == ecnt, (q, cnt[q], ecnt)
            assert np.array_equal(ids[q], eid), (q, ids[q][:8], eid[:8])
            assert np.array_equal(bits(sc[q]), bits(esc)), (q, sc[q][:8], esc[:8])


def seam_corpus(vg, ctx, n, seed=3):
    T = vg.BM25_TILE_DOCS
    rng = np.random.default_rng(seed + n)
    doc_len = rng.integers(1, 40, n)
    if n > 5:
        doc_len[5] = 0                                               # a doc of length 0 (it keeps its postings)
    everyone = [(d, 1 + (d * 7) % 5) for d in range(n)]              # a term listing every doc
    edges = sorted({d for t in range(0, n, T) for d in (t, min(t + T - 1, n - 1))})
    first_tile_only = [(d, 2) for d in (3, 10, T - 2) if d < min(n, T)] or [(0, 2)]   # nothing in the other tiles
    some = sorted(rng.choice(n, size=min(n, 300), replace=False).tolist())
    lists = [everyone, [(d, 3) for d in edges], first_tile_only, [(d, int(rng.integers(1, 9))) for d in some]]
    return Corpus(vg, ctx, n, lists, doc_len)


@pytest.mark.parametrize("which", ["one", "T-1", "T", "T+1", "2T+3"])
def test_tile_seams(vg, ctx, which):
    T = vg.BM25_TILE_DOCS
    n = {"one": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[which]
    c = seam_corpus(vg, ctx, n)
    c.check([[1], [2], [1, 2, 3], [3, 0, 1], [0]], 10)


K_ORDER = 60   # every doc of order_corpus


def order_corpus(vg, ctx):
    rng = np.random.default_rng(11)
    n = 60
    lists = [[(d, int(rng.integers(1, 6))) for d in range(n)] for _ in range(3)]
    return Corpus(vg, ctx, n, lists, rng.integers(5, 30, n))


def test_term_order_and_a_duplicated_term(vg, ctx):
    """The caller's idf doubles of three terms are searched on the CPU until the float64 sums, and with them the answers, differ by
    the order the terms are added in: every permutation must match the reference for THAT order."""
    c = order_corpus(vg, ctx)
    chosen = None
    for e in range(40, 60):          # (+a, b, -a): where a doc holds terms 0 and 2 equally often, b's term is absorbed or not
        w = [2.0 ** e * 1.25, 1.3, -(2.0 ** e) * 1.25]
        answers = set()
        for p in itertools.permutations(range(3)):
            ids, sc, _ = c.expect(list(p), [w[t] for t in p], K_ORDER)
            answers.add(tuple(ids.tolist()) + tuple(bits(sc).tolist()))
        if len(answers) >= 2:
            chosen = w
            break
    assert chosen is not None, "no idf triple whose sum depends on the order was found"
    queries = [[(t, chosen[t]) for t in p] for p in itertools.permutations(range(3))]
    c.check(queries, K_ORDER)
    c.check([[0, 0], [1, 2, 1]], 7)                                  # a duplicated term is a second iterator: it adds twice


def tie_corpus(vg, ctx, tfs):
    """one term; doc d holds it tfs[d] times; every doc has the same length: equal tf = equal score bits"""
    n = len(tfs)
    return Corpus(vg, ctx, n, [[(d, tf) for d, tf in enumerate(tfs)]], [10] * n)


def test_ties_follow_the_heap(vg, ctx):
    c = tie_corpus(vg, ctx, [1] * 20)
    c.check([[0]], 5)                                                # 20 identical docs, k = 5
    c2 = tie_corpus(vg, ctx, [1, 1, 2])
    off, terms, idfs = c2.arrays([[0]])
    ids, _, cnt = c2.bm.search(off, terms, idfs, 2)
    assert ids[0].tolist() == [2, 1] and cnt[0] == 2                 # [C, B]: (score desc, doc asc) would say [C, A]
    c2.check([[0]], 2)
    c3 = tie_corpus(vg, ctx, [3, 1, 5, 3, 4, 1])                     # k = 3: the 3rd and the 4th best are equal
    before = c3.bm.replayed()
    c3.check([[0]], 3)
    assert c3.bm.replayed() == before + 1


def test_ties_below_the_boundary_are_not_replayed(vg, ctx):
    c = tie_corpus(vg, ctx, [2, 1, 5, 1, 4, 2, 3, 1])                # k = 3: 5, 4, 3 are distinct, the ties lie below
    before = c.bm.replayed()
    c.check([[0]], 3)
    assert c.bm.replayed() == before


@pytest.fixture(scope="module")
def big(vg, ctx):
    rng = np.random.default_rng(21)
    n, hits = 4000, 3000
    docs = sorted(rng.choice(n, size=hits, replace=False).tolist())
    other = sorted(rng.choice(n, size=500, replace=False).tolist())
    lists = [[(d, int(rng.integers(1, 60))) for d in docs], [(d, int(rng.integers(1, 4))) for d in other]]
    return Corpus(vg, ctx, n, lists, rng.integers(1, 200, n)), hits


@pytest.mark.parametrize("k", ["1", "hits-1", "hits", "hits+5", "1000"])
def test_result_sizes(big, k):
    c, hits = big
    k = {"1": 1, "hits-1": hits - 1, "hits": hits, "hits+5": hits + 5, "1000": 1000}[k]
    c.check([[0]], k)


def test_empty_and_unknown_queries(vg, ctx, big):
    c, _ = big
    c.check([[], [7], [INV], [1, 9, 0], []], 6)                      # no terms; ids the dictionary does not have
    ids, sc, cnt = c.bm.search(np.zeros(1, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.float64), 4)   # nq = 0
    assert ids.shape == (0, 4) and cnt.shape == (0,)


def test_query_chunks(vg, ctx, big):
    c, _ = big
    queries = [[0], [1], [1, 0], [0, 1], [], [0], [1], [0, 0], [1], [0], [1, 1], [0]]
    hooks.set_hook("VG_BM25_SMALL_SCRATCH", 1)                       # 64 KiB of keys: two 3000-hit queries per chunk
    try:
        c.check(queries, 20)
    finally:
        hooks.set_hook("VG_BM25_SMALL_SCRATCH", 0)
    c.check(queries, 20)


def test_device_buffers_at_odd_offsets_on_a_callers_stream(vg, ctx, big):
    c, _ = big
    k = 9
    queries = [[0, 1], [1], [0]]
    stream = torch.cuda.Stream()

    def run(off, terms, idfs):
        with torch.cuda.stream(stream):
            d_off = devbuf.offset_like(off, 4)
            d_terms = devbuf.offset_like(terms, 4)
            flat = torch.empty(idfs.size + 1, dtype=torch.float64, device="cuda")
            d_idf = flat[1:]
            d_idf.copy_(torch.from_numpy(idfs))
            assert d_idf.data_ptr() % 16 != 0 and d_idf.is_contiguous()
            out = (devbuf.offset_like(np.zeros((len(queries), k), np.uint32), 4), devbuf.offset_like(np.zeros((len(queries), k), np.float32), 4),
                   devbuf.offset_like(np.zeros(len(queries), np.int32), 4))
            res = c.bm.search(d_off, d_terms, d_idf, k, out=out, stream=stream)
        stream.synchronize()
        return res
    c.check(queries, k, run=run)


def test_doc_to_id_is_a_permutation(vg, ctx):
    rng = np.random.default_rng(8)
    n = 500
    lists = [[(d, int(rng.integers(1, 20))) for d in range(0, n, 2)], [(d, int(rng.integers(1, 20))) for d in range(0, n, 3)]]
    c = Corpus(vg, ctx, n, lists, rng.integers(1, 50, n), doc_to_id=rng.permutation(n) + 1000)
    c.check([[0, 1], [1], [0]], 25)
    c.check([[0]], 400)                                              # k > hits, the replay's ids go through the map too
    assert c.bm.stats() == {"docs": n, "terms": 2, "postings": 250 + 167, "bytes": 3 * 8 + 417 * 8 + n * 4 + n * 4}


def test_refusals_name_the_number(vg, ctx, big):
    c, _ = big
    off, terms, idfs = c.arrays([[0]])
    with pytest.raises(vg.VecgoHipError) as e:
        c.bm.search(off, terms, idfs, 16385)
    assert e.value.status == UNSUPPORTED and "16385" in e.value.message
    c.bm.search(off, terms, idfs, 16384)                             # the limit itself is served
    off, terms, idfs = c.arrays([[0] * 65])
    with pytest.raises(vg.VecgoHipError) as e:
        c.bm.search(off, terms, idfs, 5)
    assert e.value.status == UNSUPPORTED and "65" in e.value.message
    c.check([[0] * 64], 5)
    with pytest.raises(vg.VecgoHipError) as e:                       # a descending host list names its term
        vg.Bm25(ctx, np.asarray([0, 1, 3], np.int64), np.asarray([0, 2, 1], np.uint32), np.ones(3, np.uint32), np.ones(3, np.uint32), 3, 3)
    assert e.value.status == INVALID_ARG and "term 1" in e.value.message
    with pytest.raises(vg.VecgoHipError) as e:
        vg.Bm25(ctx, np.asarray([0, 1], np.int64), np.zeros(1, np.uint32), np.ones(1, np.uint32), np.ones(1, np.uint32), 1, 0)
    assert e.value.status == INVALID_ARG and "doc_count = 0" in e.value.message
