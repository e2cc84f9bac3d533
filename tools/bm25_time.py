"""Hybrid search at serving size: DOCS docs (default 1M), a Zipf vocabulary of 100k terms, about 60 distinct terms per doc,
1024 queries of 4 terms drawn from the same distribution, k = 50 (HybridSearch's max(2k, 50) for k <= 25).  From one run:
  bm25_ms      vg_bm25_search, every buffer on the device except the query term arrays (the call reads those on the host),
               by device events: median / min / max of REPS calls after WARMUP
  rrf_ms       vg_rrf_fuse of two [1024, 50] lists on the device, the same way
  hybrid_ms    vecgo_amd.hybrid_search (search_flat over DOCS x 768 + the BM25 leg + the fusion on one stream) for a final k = 10
  postings_bytes / floor_ms / floor_fraction   the posting entries the batch's terms name (8 bytes each: doc, tf) over the
               chip's measured streaming rate, and that floor over bm25_ms
  replayed_share   the queries the tie replay answered (vg_bm25_replayed) over the queries searched
  stage_ms     one call split by the library's profile scopes: scoring, selection (with the tie test), replay
  numpy_ms     the same batch in numpy float64 on min(16, usable) cores (a thread pool; per query one scatter-add per term in
               term order, then argpartition for the top k — no heap: a timing yardstick, not the tie order), once
A handful of queries are first compared with tests/bm25_ref.py's heap, ids and score bits.  One JSON line.  A run without a
GPU fails.
Usage: python tools/bm25_time.py [docs] [nq]"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STREAM_TBS = 6.29   # float4 copy on an MI355X: the rate a streaming kernel can reach
WARMUP, REPS = 2, 10
VOCAB, TOKENS, QTERMS, K, DIM = 100_000, 72, 4, 50, 768


def corpus(docs, rng):
    """CSR postings of `docs` documents of TOKENS Zipf draws each"""
    p = 1.0 / np.arange(1, VOCAB + 1)
    cdf = np.cumsum(p / p.sum())
    tok = np.minimum(np.searchsorted(cdf, rng.random(docs * TOKENS)), VOCAB - 1).astype(np.int64)
    key = (tok << 32) | np.repeat(np.arange(docs, dtype=np.int64), TOKENS)      # (term, doc): sorted = CSR by term, docs ascending
    uniq, tf = np.unique(key, return_counts=True)
    term = (uniq >> 32).astype(np.int64)
    term_off = np.zeros(VOCAB + 1, np.int64)
    np.cumsum(np.bincount(term, minlength=VOCAB), out=term_off[1:])
    doc_len = np.full(docs, TOKENS, np.uint32)
    return term_off, (uniq & 0xFFFFFFFF).astype(np.uint32), tf.astype(np.uint32), doc_len, cdf


def main():
    import torch

    import vecgo_amd as vg
    from tests import bm25_ref as ref
    docs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    if not torch.cuda.is_available():
        raise SystemExit("bm25_time: no GPU")
    rng = np.random.default_rng(1)
    t0 = time.time()
    term_off, post_doc, post_tf, doc_len, cdf = corpus(docs, rng)
    # doc lengths vary as real ones do: the postings stay, the length is what the score divides by
    doc_len = rng.integers(TOKENS // 2, TOKENS * 2, docs).astype(np.uint32)
    total = int(doc_len.sum())
    print(f"corpus: {post_doc.size} postings, {post_doc.size / docs:.1f} distinct terms per doc, {time.time() - t0:.0f} s", flush=True)
    df = np.diff(term_off)
    q_terms = np.minimum(np.searchsorted(cdf, rng.random(nq * QTERMS)), VOCAB - 1).astype(np.uint32)
    q_off = (np.arange(nq + 1) * QTERMS).astype(np.int32)
    q_idf = np.asarray([ref.compute_idf(docs, int(df[t])) for t in q_terms], np.float64)
    ctx = vg.Context(0)
    bm = vg.Bm25(ctx, term_off, post_doc, post_tf, doc_len, total, docs)
    d_terms = torch.from_numpy(q_terms.view(np.int32)).cuda()
    d_idf = torch.from_numpy(q_idf).cuda()
    out = (torch.empty((nq, K), dtype=torch.int32, device="cuda"), torch.empty((nq, K), dtype=torch.float32, device="cuda"),
           torch.zeros(nq, dtype=torch.int32, device="cuda"))

    def timed(fn, reps=REPS):
        ms = []
        for i in range(WARMUP + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= WARMUP:
                ms.append(a.elapsed_time(b))
        return {"median": round(float(np.median(ms)), 3), "min": round(float(min(ms)), 3), "max": round(float(max(ms)), 3)}

    def search():
        return bm.search(q_off, d_terms, d_idf, K, out=out)

    # a handful of queries against the reference's heap first
    ids, sc, cnt = search()
    ids, sc, cnt = ids.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy()
    rare = np.argsort([int(df[q_terms[q * QTERMS:(q + 1) * QTERMS]].sum()) for q in range(nq)])[:4]
    for q in rare:
        s = slice(q * QTERMS, (q + 1) * QTERMS)
        eid, esc, ecnt = ref.csr_search(term_off, post_doc, post_tf, doc_len, total, docs, q_terms[s], q_idf[s], K)
        assert ecnt == cnt[q] and np.array_equal(eid, ids[q]) and np.array_equal(esc.view(np.uint32), sc[q].view(np.uint32)), int(q)
    print("checked against the reference's heap", flush=True)
    before = bm.replayed()
    bm25 = timed(search)
    replayed = (bm.replayed() - before) / ((WARMUP + REPS) * nq)
    print("bm25", bm25, "replayed share", replayed, flush=True)
    ctx.profile_enable(True)   # the stages of one call by the library's event pairs (bm25_select includes the tie test)
    search()
    stages = {name: round(ctx.profile_read(name)[1], 3) for name in ("bm25_score", "bm25_select", "bm25_replay")}
    ctx.profile_enable(False)
    print("stages", stages, flush=True)

    a_ids = torch.from_numpy(rng.integers(0, docs, (nq, K)).astype(np.int32)).cuda()
    a_cnt = torch.full((nq,), K, dtype=torch.int32, device="cuda")
    f_out = (torch.empty((nq, 10), dtype=torch.int32, device="cuda"), torch.empty((nq, 10), dtype=torch.float32, device="cuda"),
             torch.zeros(nq, dtype=torch.int32, device="cuda"))
    rrf = timed(lambda: vg.rrf_fuse(ctx, a_ids, a_cnt, out[0], out[2], 10, out=f_out))
    print("rrf", rrf, flush=True)

    idx = vg.Index(ctx, docs, DIM, vg.Metric.L2)
    idx.set_vectors(torch.randn((docs, DIM), dtype=torch.float32, device="cuda"))
    queries = torch.randn((nq, DIM), dtype=torch.float32, device="cuda")
    hybrid = timed(lambda: vg.hybrid_search(idx, bm, queries, q_off, d_terms, d_idf, 10), reps=5)
    print("hybrid", hybrid, flush=True)

    k1_b_avgdl = 0.9 / (total / docs)

    def numpy_query(q):
        acc = np.zeros(docs, np.float64)
        for t, w in zip(q_terms[q * QTERMS:(q + 1) * QTERMS], q_idf[q * QTERMS:(q + 1) * QTERMS]):
            a, b = term_off[t], term_off[t + 1]
            d, tf = post_doc[a:b], post_tf[a:b].astype(np.float64)
            acc[d] += w * ((tf * 2.2) / (tf + 0.3 + k1_b_avgdl * doc_len[d]))
        hit = np.flatnonzero(acc > 0)
        s = acc[hit].astype(np.float32)
        top = np.argpartition(-s, min(K, s.size) - 1)[:K] if s.size else hit
        return hit[top]

    workers = min(16, len(os.sched_getaffinity(0)))
    t0 = time.time()
    with ThreadPoolExecutor(workers) as pool:
        list(pool.map(numpy_query, range(nq)))
    numpy_ms = (time.time() - t0) * 1e3
    postings = int(df[q_terms].sum())
    floor_ms = postings * 8 / (STREAM_TBS * 1e12) * 1e3
    print(json.dumps({"docs": docs, "nq": nq, "k": K, "postings_total": int(post_doc.size), "bm25_ms": bm25, "rrf_ms": rrf, "hybrid_ms": hybrid,
                      "postings_bytes": postings * 8, "floor_ms": round(floor_ms, 4), "floor_fraction": round(floor_ms / bm25["median"], 4),
                      "replayed_share": round(replayed, 4), "stage_ms": stages, "numpy_ms": round(numpy_ms, 1), "numpy_workers": workers,
                      "resident_bytes": bm.stats()["bytes"]}))


if __name__ == "__main__":
    main()
