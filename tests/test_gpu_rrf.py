"""vg_rrf_fuse and hybrid_search on the device against tests/bm25_ref.py: score bits against numpy float32, scores
non-increasing, ids ascending inside equal scores, the set the reference's."""
import json

import numpy as np
import pytest
import torch

from oracle import oracle as o
from tests import bm25_ref as ref

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
UNSUPPORTED = -5


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


def pad(lists, stride):
    ids = np.full((len(lists), stride), INV, np.uint32)
    for q, li in enumerate(lists):
        ids[q, :len(li)] = li
    return ids, np.asarray([len(li) for li in lists], np.int32)


def check(vg, ctx, a_lists, b_lists, rrf_k, k, stride=None, device=False):
    stride = stride or max(1, max(len(li) for li in a_lists + b_lists))
    a, ca = pad(a_lists, stride)
    b, cb = pad(b_lists, stride)
    args = [torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda() for x in (a, ca, b, cb)] if device else [a, ca, b, cb]
    ids, sc, cnt = vg.rrf_fuse(ctx, args[0], args[1], args[2], args[3], k, rrf_k=rrf_k)
    if device:
        ids, sc, cnt = ids.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy()
    for q in range(len(a_lists)):
        eid, esc, ecnt = ref.rrf_fuse(a[q, :ca[q]], b[q, :cb[q]], rrf_k, k)
        assert cnt[q] == ecnt, (q, cnt[q], ecnt)
        assert np.array_equal(bits(sc[q]), bits(esc)), (q, sc[q][:6], esc[:6])           # numpy float32, bit for bit
        n = int(cnt[q])
        assert np.all(sc[q, 1:n] <= sc[q, :n - 1])                                       # non-increasing
        same = sc[q, 1:n] == sc[q, :n - 1]
        assert np.all(ids[q, 1:n][same] > ids[q, :n - 1][same])                          # ids ascending inside equal scores
        assert set(ids[q, :n].tolist()) == set(eid[:n].tolist())
        assert np.array_equal(ids[q], eid)
        assert np.all(ids[q, n:] == INV) and np.all(np.isneginf(sc[q, n:]))


@pytest.mark.parametrize("rrf_k", [0, 60])
@pytest.mark.parametrize("device", [False, True])
def test_rrf_cases(vg, ctx, rrf_k, device):
    a = [[1, 2, 3, 4], [5, 6, 7], [1, 2, 3, 4, 5], [], [9, 8], [4, INV, 6], [7, 3, 7, 2], [1, 2]]
    b = [[10, 11, 12], [5, 6, 7], [4, 5, 6, 1], [3, 1, 2], [], [INV, 6, 5], [2, 9], [5, 1, 5, 5]]
    # disjoint; identical; partial overlap; A empty; B empty; INVALID_ID padding inside; a repeated id in A (last rank wins); in B (adds)
    for k in (2, 5, 20):                                             # below and above the union's size
        check(vg, ctx, a, b, rrf_k, k, stride=7, device=device)      # counts below the stride


def test_rrf_one_side_missing(vg, ctx):
    a, ca = pad([[3, 1, 2], [5]], 4)
    ids, sc, cnt = vg.rrf_fuse(ctx, a, ca, None, None, 3)
    for q in range(2):
        eid, esc, ecnt = ref.rrf_fuse(a[q, :ca[q]], [], 60, 3)
        assert np.array_equal(ids[q], eid) and np.array_equal(bits(sc[q]), bits(esc)) and cnt[q] == ecnt
    ids, sc, cnt = vg.rrf_fuse(ctx, None, None, a, ca, 3)
    for q in range(2):
        eid, esc, ecnt = ref.rrf_fuse([], a[q, :ca[q]], 60, 3)
        assert np.array_equal(ids[q], eid) and np.array_equal(bits(sc[q]), bits(esc)) and cnt[q] == ecnt


def test_rrf_limit(vg, ctx):
    rng = np.random.default_rng(2)
    a = rng.permutation(20000)[:8192].astype(np.uint32)
    b = rng.permutation(20000)[:8193].astype(np.uint32)
    check(vg, ctx, [a.tolist()], [b[:8192].tolist()], 60, 100)       # 16384 entries are served
    ai, ca = pad([a.tolist()], 8193)
    bi, cb = pad([b.tolist()], 8193)
    with pytest.raises(vg.VecgoHipError) as e:
        vg.rrf_fuse(ctx, ai, ca, bi, cb, 100)
    assert e.value.status == UNSUPPORTED and "16385" in e.value.message


def corpus_index(vg, ctx, texts, vectors):
    mem = ref.MemoryIndex()
    for i, t in enumerate(texts):
        mem.add(i, t)                                                # primary key = row id
    vocab, term_off, post_doc, post_tf, doc_len, total, count, doc_to_pk = mem.export_csr()
    bm = vg.Bm25(ctx, term_off, post_doc, post_tf, doc_len, total, count, doc_to_pk)
    idx = vg.Index(ctx, len(texts), vectors.shape[1], vg.Metric.L2)
    idx.set_vectors(vectors)
    return mem, vocab, bm, idx


def hybrid_expect(mem, vectors, query, text, k, rrf_k):
    vk = max(2 * k, 50)
    vid, _ = o.flat_search_f32(vectors, vectors.shape[1], query, min(vk, len(vectors)))
    lex = mem.search(text, vk, sort=True)
    return ref.rrf_fuse(np.asarray(vid, np.uint32), np.asarray([pk for pk, _ in lex], np.uint32), rrf_k, k)


def test_hybrid_search_on_the_reference_corpus(vg, ctx, golden_dir):
    kat = json.loads((golden_dir / "bm25_kats.json").read_text())["hybrid"]
    rows = kat["rows"]
    vectors = np.asarray([r["vector"] for r in rows], np.float32)
    mem, vocab, bm, idx = corpus_index(vg, ctx, [r["text"] for r in rows], vectors)
    for s in kat["searches"]:
        q = np.asarray([s["vector"]], np.float32)
        off, terms, idfs = mem.query_arrays([s["text"]], vocab)
        ids, sc, cnt = vg.hybrid_search(idx, bm, q, off, terms, idfs, s["k"], rrf_k=s["rrf_k"])
        ids, sc, cnt = ids.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy()
        pks = [rows[i]["id"] for i in ids[0, :cnt[0]]]
        if "first" in s["expect"]:
            assert pks[0] == s["expect"]["first"]
        for want in s["expect"].get("contains", []):
            assert want in pks
        eid, esc, ecnt = hybrid_expect(mem, vectors, q[0], s["text"], s["k"], s["rrf_k"])
        assert cnt[0] == ecnt and np.array_equal(ids[0], eid) and np.array_equal(bits(sc[0]), bits(esc))


def test_hybrid_search_end_to_end(vg, ctx):
    rng = np.random.default_rng(17)
    n, dim, nv, nq, k = 2000, 32, 300, 8, 10
    words = [f"w{i}" for i in range(nv)]
    p = 1.0 / np.arange(1, nv + 1)
    p /= p.sum()
    texts = [" ".join(rng.choice(words, size=int(rng.integers(3, 25)), p=p)) for _ in range(n)]
    vectors = rng.standard_normal((n, dim)).astype(np.float32)
    mem, vocab, bm, idx = corpus_index(vg, ctx, texts, vectors)
    queries = rng.standard_normal((nq, dim)).astype(np.float32)
    qtexts = [" ".join(rng.choice(words, size=3, p=p)) for _ in range(nq - 1)] + ["nosuchword"]
    off, terms, idfs = mem.query_arrays(qtexts, vocab)
    ids, sc, cnt = vg.hybrid_search(idx, bm, queries, off, terms, idfs, k)
    ids, sc, cnt = ids.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy()
    for q in range(nq):
        eid, esc, ecnt = hybrid_expect(mem, vectors, queries[q], qtexts[q], k, 60)
        assert cnt[q] == ecnt, q
        assert np.array_equal(ids[q], eid), (q, ids[q], eid)
        assert np.array_equal(bits(sc[q]), bits(esc)), q
