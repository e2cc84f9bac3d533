"""lexical/bm25 MemoryIndex (bm25.go) and the fusion loop of Engine.HybridSearch (engine.go:1560-1602) restated in Python:
the tokeniser, Add / Delete with the free list, the document-at-a-time walk in float64 and candidateHeap exactly as written.
Python floats are IEEE doubles and nothing here is fused; float32 values are numpy's.  What vg_bm25_search / vg_rrf_fuse
(include/vecgo_hip.h) are compared against, bit for bit."""
import math

import numpy as np

K1_PLUS_1 = 2.2   # bm25.go:315-317: k1 + 1, k1 * (1 - b), k1 * b are exact CONSTANT expressions in Go (k1 = 1.2, b = 0.75),
K1_1B = 0.3       # rounded to float64 once: 2.2, 0.3, 0.9 (float64(1.2) + 1 would round differently)
K1_B = 0.9
INVALID_ID = 0xFFFFFFFF

# unicode.IsSpace
_SPACE = {0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000} | set(range(0x2000, 0x200B))


def _lower_rune(ch):
    """unicode.ToLower maps a rune to ONE rune (Python's str.lower may give several: then the rune stays)"""
    low = ch.lower()
    return low if len(low) == 1 else ch


def tokenize(text):
    """MemoryIndex.tokenize (bm25.go:90-178): the ASCII path splits at bytes <= ' ' and lowers A-Z; other text splits at
    unicode.IsSpace and lowers rune by rune"""
    if all(ord(c) < 128 for c in text):
        out, cur = [], []
        for c in text:
            if c <= " ":
                if cur:
                    out.append("".join(cur))
                    cur = []
            else:
                cur.append(chr(ord(c) + 32) if "A" <= c <= "Z" else c)
        if cur:
            out.append("".join(cur))
        return out
    out, cur = [], []
    for c in text:
        if ord(c) in _SPACE:
            if cur:
                out.append("".join(cur))
                cur = []
        else:
            cur.append(_lower_rune(c))
    if cur:
        out.append("".join(cur))
    return out


def compute_idf(doc_count, df):
    """computeIDF (bm25.go:383-387); the tests hand these same doubles to the device"""
    n_docs, n = float(doc_count), float(df)
    return math.log(1 + (n_docs - n + 0.5) / (n + 0.5))


# ---- candidateHeap (bm25.go:394-441): items are (float32 score, id); scores alone are compared -----------------------------
def heap_up(h, j):
    while True:
        i = int((j - 1) / 2)   # Go's integer division truncates toward zero: the root is its own parent
        if i == j or h[j][0] >= h[i][0]:
            break
        h[i], h[j] = h[j], h[i]
        j = i


def heap_down(h, i0, n):
    i = i0
    while True:
        j1 = 2 * i + 1
        if j1 >= n or j1 < 0:
            break
        j = j1
        j2 = j1 + 1
        if j2 < n and h[j2][0] < h[j1][0]:
            j = j2
        if h[j][0] >= h[i][0]:
            break
        h[i], h[j] = h[j], h[i]
        i = j


def heap_push(h, x):
    h.append(x)
    heap_up(h, len(h) - 1)


def heap_pop(h):
    root = h[0]
    h[0] = h[-1]
    h.pop()
    if h:
        heap_down(h, 0, len(h))
    return root


def heap_topk(scored, k):
    """the heap part of Search (bm25.go:363-378) over (float64 score, id) in the walk's order -> [(id, float32 score)] best first"""
    h = []
    for score, pk in scored:
        if score > 0:
            s32 = np.float32(score)
            if len(h) < k:
                heap_push(h, (s32, pk))
            elif s32 > h[0][0]:
                h[0] = (s32, pk)
                heap_down(h, 0, len(h))
    out = [None] * len(h)
    for i in range(len(h) - 1, -1, -1):
        s, pk = heap_pop(h)
        out[i] = (pk, s)
    return out


def daat_scores(lists, idfs, doc_lengths, total_length, doc_count):
    """the walk of bm25.go:314-360: lists = one posting list [(doc, tf), ...] per iterator, IN THE ORDER GIVEN (not sorted
    here: an unsorted list makes the walk meet a doc more than once) -> [(doc, float64 score)] in the walk's order"""
    with np.errstate(all="ignore"):
        avg_dl = np.float64(total_length) / np.float64(doc_count)
        k1_b_avgdl = float(np.float64(K1_B) / avg_dl)
    pos = [0] * len(lists)
    out = []
    while True:
        min_doc = INVALID_ID
        for li, p in zip(lists, pos):
            if p < len(li) and li[p][0] < min_doc:
                min_doc = li[p][0]
        if min_doc == INVALID_ID:
            break
        score = 0.0
        doc_len = float(doc_lengths[min_doc])
        for i, li in enumerate(lists):
            if pos[i] < len(li) and li[pos[i]][0] == min_doc:
                tf = float(li[pos[i]][1])
                num = tf * K1_PLUS_1
                denom = tf + K1_1B + k1_b_avgdl * doc_len
                score += idfs[i] * (num / denom)
                pos[i] += 1
        out.append((min_doc, score))
    return out


class MemoryIndex:
    def __init__(self):
        self.pk_to_doc, self.doc_to_pk, self.free_ids = {}, [], []
        self.doc_lengths, self.inverted, self.doc_terms = [], {}, []
        self.total_length, self.doc_count = 0, 0

    def add(self, pk, text):
        if pk in self.pk_to_doc:
            self.delete(pk)
        if self.free_ids:
            doc = self.free_ids.pop()
            self.doc_to_pk[doc] = pk
        else:
            doc = len(self.doc_to_pk)
            self.doc_to_pk.append(pk)
            self.doc_lengths.append(0)
            self.doc_terms.append(None)
        self.pk_to_doc[pk] = doc
        tf = {}
        length = 0
        for t in tokenize(text):
            length += 1
            tf[t] = tf.get(t, 0) + 1
        self.doc_lengths[doc] = length
        self.total_length += length
        self.doc_count += 1
        for t, c in tf.items():
            self.inverted.setdefault(t, []).append((doc, c))
        self.doc_terms[doc] = list(tf)

    def delete(self, pk):
        doc = self.pk_to_doc.get(pk)
        if doc is None:
            return
        for t in self.doc_terms[doc]:
            li = self.inverted[t]
            for i, p in enumerate(li):
                if p[0] == doc:
                    li[i] = li[-1]   # swap-remove (bm25.go:252-254): the list may now be out of order
                    li.pop()
                    break
            if not li:
                del self.inverted[t]
        self.total_length -= self.doc_lengths[doc]
        self.doc_count -= 1
        self.doc_lengths[doc] = 0
        self.doc_to_pk[doc] = 0
        self.doc_terms[doc] = None
        del self.pk_to_doc[pk]
        self.free_ids.append(doc)

    def iterators(self, text, sort=False):
        """(posting lists, idfs) of the query's tokens that have a list, in token order; sort: ascending docs (the shim's form)"""
        lists, idfs = [], []
        for t in tokenize(text):
            li = self.inverted.get(t)
            if not li:
                continue
            lists.append(sorted(li) if sort else list(li))
            idfs.append(compute_idf(self.doc_count, len(li)))
        return lists, idfs

    def search(self, text, k, sort=False):
        """MemoryIndex.Search -> [(pk, float32 score)] best first"""
        if self.doc_count == 0:
            return []
        lists, idfs = self.iterators(text, sort)
        if not lists:
            return []
        scored = daat_scores(lists, idfs, self.doc_lengths, self.total_length, self.doc_count)
        return heap_topk([(s, self.doc_to_pk[d]) for d, s in scored], k)

    def export_csr(self):
        """what vg_bm25_create takes: ({term: id} by sorted term, term_off int64, post_doc, post_tf (ascending docs), doc_len,
        total_length, doc_count, doc_to_pk)"""
        terms = sorted(self.inverted)
        off, docs, tfs = [0], [], []
        for t in terms:
            for d, c in sorted(self.inverted[t]):
                docs.append(d)
                tfs.append(c)
            off.append(len(docs))
        return ({t: i for i, t in enumerate(terms)}, np.asarray(off, np.int64), np.asarray(docs, np.uint32), np.asarray(tfs, np.uint32),
                np.asarray(self.doc_lengths, np.uint32), self.total_length, self.doc_count, np.asarray(self.doc_to_pk, np.uint32))

    def query_arrays(self, texts, vocab):
        """(q_term_off int32, q_terms uint32, q_idf float64) of a batch of query texts: the tokens the dictionary has"""
        off, terms, idfs = [0], [], []
        for text in texts:
            for t in tokenize(text):
                if t in vocab:
                    terms.append(vocab[t])
                    idfs.append(compute_idf(self.doc_count, len(self.inverted[t])))
            off.append(len(terms))
        return np.asarray(off, np.int32), np.asarray(terms, np.uint32), np.asarray(idfs, np.float64)


def csr_search(term_off, post_doc, post_tf, doc_len, total_length, doc_count, terms, idfs, k, doc_to_id=None):
    """MemoryIndex.Search over CSR arrays for one query's term ids / idfs -> (ids uint32 [k], scores float32 [k], count), padded
    as vg_bm25_search pads"""
    lists, ws = [], []
    for t, w in zip(terms, idfs):
        t = int(t)
        if t >= len(term_off) - 1 or term_off[t + 1] == term_off[t]:
            continue
        a, b = int(term_off[t]), int(term_off[t + 1])
        lists.append(list(zip(post_doc[a:b].tolist(), post_tf[a:b].tolist())))
        ws.append(float(w))
    scored = daat_scores(lists, ws, doc_len, total_length, doc_count) if lists else []
    res = heap_topk([(s, int(doc_to_id[d]) if doc_to_id is not None else d) for d, s in scored], k)
    ids = np.full(k, INVALID_ID, np.uint32)
    sc = np.full(k, -np.inf, np.float32)
    for i, (pk, s) in enumerate(res):
        ids[i], sc[i] = pk, s
    return ids, sc, len(res)


def rrf_fuse(a_ids, b_ids, rrf_k, k):
    """engine.go:1560-1602 with ties DEFINED as ascending id; INVALID_ID entries are skipped (they keep their rank)
    -> (ids uint32 [k], scores float32 [k], count)"""
    final = {}
    for rank, i in enumerate(a_ids):
        if int(i) != INVALID_ID:
            final[int(i)] = np.float32(1.0) / np.float32(rrf_k + rank + 1)
    for rank, i in enumerate(b_ids):
        if int(i) != INVALID_ID:
            final[int(i)] = np.float32(final.get(int(i), np.float32(0.0)) + np.float32(1.0) / np.float32(rrf_k + rank + 1))
    order = sorted(final.items(), key=lambda kv: (-float(kv[1]), kv[0]))[:k]
    ids = np.full(k, INVALID_ID, np.uint32)
    sc = np.full(k, -np.inf, np.float32)
    for j, (i, s) in enumerate(order):
        ids[j], sc[j] = i, s
    return ids, sc, len(order)
