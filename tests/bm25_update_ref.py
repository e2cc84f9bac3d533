"""vg_bm25_update (include/vecgo_hip.h) restated in numpy on CSR arrays: deletes, then adds, every list ascending by doc, term
ids stable, sizes that never shrink.  Also the host-side checks of the call as a few lines of Python, and the driver the tests
replay a script of MemoryIndex writes through: it turns batches of Add / Delete into the call's arrays the way the cgo shim
does (append-only dictionary, doc ids from the reference's free list).  tests/test_bm25_update_cpu.py pins all of it against
tests/bm25_ref.py's MemoryIndex; the GPU tests compare the device's image with it bit for bit."""
import numpy as np

from tests import bm25_ref as ref


class Refused(ValueError):
    """what the call answers with VG_ERR_INVALID_ARG; .what names the rule, .number the doc or term"""

    def __init__(self, what, number):
        super().__init__(f"{what}: {number}")
        self.what, self.number = what, number


class Csr:
    """the image: term_off int64 [n_terms + 1], post_doc / post_tf uint32, doc_len uint32 [n_docs], doc_to_id uint32 or None"""

    def __init__(self, term_off=None, post_doc=None, post_tf=None, doc_len=None, doc_to_id=None, mapped=None):
        self.term_off = np.zeros(1, np.int64) if term_off is None else np.asarray(term_off, np.int64)
        self.post_doc = np.zeros(0, np.uint32) if post_doc is None else np.asarray(post_doc, np.uint32)
        self.post_tf = np.zeros(0, np.uint32) if post_tf is None else np.asarray(post_tf, np.uint32)
        self.doc_len = np.zeros(0, np.uint32) if doc_len is None else np.asarray(doc_len, np.uint32)
        self.mapped = (doc_to_id is not None) if mapped is None else mapped
        self.doc_to_id = None if not self.mapped else (np.zeros(0, np.uint32) if doc_to_id is None else np.asarray(doc_to_id, np.uint32))

    @property
    def n_terms(self):
        return self.term_off.size - 1

    @property
    def n_docs(self):
        return self.doc_len.size

    def arrays(self):
        return self.term_off, self.post_doc, self.post_tf, self.doc_len, self.doc_to_id


def _u32(x):
    return np.zeros(0, np.uint32) if x is None else np.asarray(x, np.uint32).reshape(-1)


def validate(csr, del_docs, add_docs, add_off, add_terms, n_docs_new, n_terms_new):
    """the checks vg_bm25_update makes on arrays in host memory, in plain Python"""
    if n_docs_new < csr.n_docs:
        raise Refused("n_docs_new shrinks", n_docs_new)
    if n_terms_new < csr.n_terms:
        raise Refused("n_terms_new shrinks", n_terms_new)
    for d in del_docs:
        if int(d) >= csr.n_docs:
            raise Refused("deleted doc out of range", int(d))
    seen = set()
    for d in add_docs:
        if int(d) >= n_docs_new:
            raise Refused("added doc out of range", int(d))
        if int(d) in seen:
            raise Refused("doc named twice", int(d))
        seen.add(int(d))
    for i in range(len(add_docs)):
        if add_off[i + 1] < add_off[i]:
            raise Refused("add_off decreases", i)
        terms = set()
        for t in add_terms[int(add_off[i]):int(add_off[i + 1])]:
            if int(t) >= n_terms_new:
                raise Refused("term out of range", int(t))
            if int(t) in terms:
                raise Refused("term named twice", int(t))
            terms.add(int(t))


def update(csr, del_docs, add_docs, add_len, add_off, add_terms, add_tf, n_docs_new, n_terms_new, add_ids=None):
    """the image after the call (a new Csr; `csr` is not changed); Refused as the call refuses"""
    del_docs, add_docs, add_len, add_terms, add_tf = _u32(del_docs), _u32(add_docs), _u32(add_len), _u32(add_terms), _u32(add_tf)
    add_off = np.zeros(1, np.int64) if add_off is None or add_docs.size == 0 else np.asarray(add_off, np.int64)
    validate(csr, del_docs, add_docs, add_off, add_terms, n_docs_new, n_terms_new)
    term_of = np.repeat(np.arange(csr.n_terms, dtype=np.int64), np.diff(csr.term_off))
    keep = ~np.isin(csr.post_doc, del_docs)
    terms = np.concatenate([term_of[keep], add_terms.astype(np.int64)])
    docs = np.concatenate([csr.post_doc[keep], np.repeat(add_docs, np.diff(add_off))])
    tfs = np.concatenate([csr.post_tf[keep], add_tf])
    order = np.lexsort((docs, terms))
    terms, docs, tfs = terms[order], docs[order], tfs[order]
    twice = np.flatnonzero((terms[1:] == terms[:-1]) & (docs[1:] == docs[:-1]))
    if twice.size:
        raise Refused("add into a live slot", int(docs[twice[0]]))
    term_off = np.concatenate([[0], np.cumsum(np.bincount(terms, minlength=n_terms_new))]).astype(np.int64)
    doc_len = np.zeros(n_docs_new, np.uint32)
    doc_len[:csr.n_docs] = csr.doc_len
    doc_len[del_docs] = 0
    doc_len[add_docs] = add_len
    doc_to_id = None
    if csr.mapped:
        doc_to_id = np.zeros(n_docs_new, np.uint32)
        doc_to_id[:csr.n_docs] = csr.doc_to_id
        doc_to_id[del_docs] = 0
        doc_to_id[add_docs] = _u32(add_ids)
    return Csr(term_off, docs.astype(np.uint32), tfs.astype(np.uint32), doc_len, doc_to_id, mapped=csr.mapped)


class Driver:
    """MemoryIndex writes gathered into batches for vg_bm25_update, as go/lexical/bm25_hip.go gathers them: the dictionary only
    grows (a term keeps its id for good), doc ids come from the reference's own allocation (its free list included)"""

    def __init__(self):
        self.mem = ref.MemoryIndex()
        self.vocab = {}            # term -> id, append-only
        self.doc_tf = {}           # doc -> {term id: tf} of the docs that hold a document
        self.touched = {}          # doc -> did it hold a document before the pending batch?

    def _touch(self, doc):
        self.touched.setdefault(doc, doc in self.doc_tf)

    def delete(self, pk):
        doc = self.mem.pk_to_doc.get(pk)
        if doc is None:
            return
        self._touch(doc)
        self.mem.delete(pk)

    def add(self, pk, text):
        if pk in self.mem.pk_to_doc:
            self.delete(pk)
        self.mem.add(pk, text)
        doc = self.mem.pk_to_doc[pk]
        self._touch(doc)
        for t in ref.tokenize(text):
            self.vocab.setdefault(t, len(self.vocab))

    def flush(self):
        """the pending batch as the call's arguments: dict(del_docs, add_docs, add_len, add_ids, add_off, add_terms, add_tf,
        n_docs, n_terms, total_length, doc_count)"""
        mem = self.mem
        del_docs = sorted(d for d, had in self.touched.items() if had)
        add_docs = [d for d in self.touched if mem.doc_terms[d] is not None]
        for d in del_docs:
            self.doc_tf.pop(d, None)
        off, terms, tfs = [0], [], []
        for d in add_docs:
            tf = {self.vocab[t]: c for t in mem.doc_terms[d] for dd, c in mem.inverted[t] if dd == d}
            self.doc_tf[d] = tf
            terms += list(tf)
            tfs += list(tf.values())
            off.append(len(terms))
        self.touched = {}
        return dict(del_docs=np.asarray(del_docs, np.uint32), add_docs=np.asarray(add_docs, np.uint32),
                    add_len=np.asarray([mem.doc_lengths[d] for d in add_docs], np.uint32),
                    add_ids=np.asarray([mem.doc_to_pk[d] for d in add_docs], np.uint32), add_off=np.asarray(off, np.int64),
                    add_terms=np.asarray(terms, np.uint32), add_tf=np.asarray(tfs, np.uint32), n_docs=len(mem.doc_to_pk),
                    n_terms=len(self.vocab), total_length=mem.total_length, doc_count=mem.doc_count)

    def lists_equal(self, csr):
        """is csr the MemoryIndex's state: every term's list sorted by doc under the append-only ids, lengths, doc -> pk?"""
        mem = self.mem
        if csr.n_terms != len(self.vocab) or csr.n_docs != len(mem.doc_to_pk):
            return False
        for t, i in self.vocab.items():
            want = sorted(mem.inverted.get(t, []))
            a, b = int(csr.term_off[i]), int(csr.term_off[i + 1])
            if list(zip(csr.post_doc[a:b].tolist(), csr.post_tf[a:b].tolist())) != want:
                return False
        return csr.doc_len.tolist() == mem.doc_lengths and (csr.doc_to_id is None or csr.doc_to_id.tolist() == mem.doc_to_pk)

    def query(self, text):
        """(term ids, idfs) of a query text: the tokens whose list is not empty (the reference deletes an emptied list)"""
        terms, idfs = [], []
        for t in ref.tokenize(text):
            li = self.mem.inverted.get(t)
            if li:
                terms.append(self.vocab[t])
                idfs.append(ref.compute_idf(self.mem.doc_count, len(li)))
        return terms, idfs


def zipf_script(seed, n_ops, n_words=40, max_batch=50):
    """batches of ("add", pk, text) / ("delete", pk) over a Zipf vocabulary: adds, deletes, replaces, one batch that deletes
    every doc (doc_count back to 0) and batches after it"""
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(n_words)]
    p = 1.0 / np.arange(1, n_words + 1)
    p /= p.sum()
    live, next_pk, batches, done = [], 1, [], 0
    emptied = False
    while done < n_ops:
        batch = []
        if not emptied and done >= n_ops // 2:
            batch = [("delete", pk) for pk in live]           # everything goes: doc_count == 0 afterwards
            live, emptied = [], True
        else:
            for _ in range(int(rng.integers(1, max_batch + 1))):
                r = rng.random()
                if live and r < 0.25:
                    batch.append(("delete", live.pop(int(rng.integers(len(live))))))
                    continue
                if live and r < 0.4:
                    pk = live[int(rng.integers(len(live)))]       # a replace: Add of a pk the index holds
                else:
                    pk, next_pk = next_pk, next_pk + 1
                    live.append(pk)
                batch.append(("add", pk, " ".join(rng.choice(words, size=int(rng.integers(1, 12)), p=p))))
        done += len(batch)
        batches.append(batch)
    return batches
