"""A write to a resident BM25 index at serving size: tools/bm25_time.py's corpus (default 1M docs, a Zipf vocabulary of 100k terms,
about 60 distinct terms per doc).  For B in 1, 1024, 65536, in one process:
  update_ms     one vg_bm25_update that deletes B docs and adds B docs (the same doc ids with freshly drawn terms: B replaces),
                every array in host memory as the cgo shim passes them; a host clock around the call, which ends in the
                call's own wait for the device: median / min / max of REPS calls after WARMUP, each with a batch of its own
  stage_ms      one more call split by the library's profile scopes: live marking, ordering the added postings, offsets, merge
  streamed_bytes / update_gbs / stream_fraction   the bytes the passes move by their shapes — 12 per old posting (doc twice, tf
                once; 8 when nothing is deleted), 8 per new posting, 24 per added posting and radix pass — over update_ms, and
                that rate over the chip's measured streaming rate
  recreate_ms   the only way the library had before to reach the same state: vg_bm25_destroy + vg_bm25_create from host
                arrays, the same clock: median / min / max of CREATE_REPS
  assemble_ms   what that way needs first, the updated CSR on the host: the old postings without the deleted docs merged with
                the added ones (numpy: isin, searchsorted, insert — no sort of the whole index), measured once
  ratio         recreate_ms / update_ms, and (assemble_ms + recreate_ms) / update_ms
After the timed updates of each B the exported image is compared with the host's assembled arrays, bit for bit.  One JSON line.
A run without a GPU fails.
Usage: python tools/bm25_update_time.py [docs]"""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
STREAM_TBS = 6.29   # float4 copy on an MI355X: the rate a streaming kernel can reach
WARMUP, REPS, CREATE_REPS = 2, 10, 3
BATCHES = (1, 1024, 65536)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return {"median": round(float(np.median(ms)), 3), "min": round(float(min(ms)), 3), "max": round(float(max(ms)), 3)}


def draw_batch(docs, cdf, rng, vocab, tokens):
    """the docs `docs` with freshly drawn terms: add_off, add_terms, add_tf (document-major)"""
    tok = np.minimum(np.searchsorted(cdf, rng.random(docs.size * tokens)), vocab - 1).astype(np.int64)
    key = (np.repeat(np.arange(docs.size, dtype=np.int64), tokens) << 32) | tok          # (doc index, term)
    uniq, tf = np.unique(key, return_counts=True)
    off = np.zeros(docs.size + 1, np.int64)
    np.cumsum(np.bincount(uniq >> 32, minlength=docs.size), out=off[1:])
    return off, (uniq & 0xFFFFFFFF).astype(np.uint32), tf.astype(np.uint32)


def assemble(term_off, post_doc, post_tf, vocab, docs, off, terms, tfs):
    """the CSR after `docs` were deleted and added again with the batch's postings: (term_off, post_doc, post_tf)"""
    term_of = np.repeat(np.arange(vocab, dtype=np.int64), np.diff(term_off))
    keep = ~np.isin(post_doc, docs)
    old_key = (term_of[keep] << 32) | post_doc[keep]
    old_tf = post_tf[keep]
    new_key = (terms.astype(np.int64) << 32) | np.repeat(docs.astype(np.int64), np.diff(off))
    order = np.argsort(new_key, kind="stable")
    new_key, new_tf = new_key[order], tfs[order]
    at = np.searchsorted(old_key, new_key)
    key = np.insert(old_key, at, new_key)
    tf = np.insert(old_tf, at, new_tf)
    out_off = np.zeros(vocab + 1, np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=vocab), out=out_off[1:])
    return out_off, (key & 0xFFFFFFFF).astype(np.uint32), tf.astype(np.uint32)


def radix_passes(n_docs, n_terms):
    return sum(1 for half in (n_docs - 1, n_terms - 1) for d in range(4) if half >> (8 * d))


def main():
    import torch

    import bm25_time
    import vecgo_amd as vg
    docs = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    if not torch.cuda.is_available():
        raise SystemExit("bm25_update_time: no GPU")
    vocab, tokens = bm25_time.VOCAB, bm25_time.TOKENS
    rng = np.random.default_rng(1)
    t0 = time.time()
    term_off, post_doc, post_tf, doc_len, cdf = bm25_time.corpus(docs, rng)
    total = int(doc_len.sum())
    print(f"corpus: {post_doc.size} postings, {time.time() - t0:.0f} s", flush=True)
    ctx = vg.Context(0)
    bm = vg.Bm25(ctx, term_off, post_doc, post_tf, doc_len, total, docs)
    other = None
    none = np.zeros(0, np.uint32)
    report = {"docs": docs, "vocab": vocab, "postings": int(post_doc.size), "batches": {}}
    for b in BATCHES:
        b = min(b, docs)
        which = np.sort(rng.choice(docs, size=b, replace=False)).astype(np.uint32)
        lens = doc_len[which]
        batches = [draw_batch(which, cdf, rng, vocab, tokens) for _ in range(WARMUP + REPS + 1)]
        ms, n_old = [], []
        for i, (off, terms, tfs) in enumerate(batches[:-1]):
            n_old.append(bm.stats()["postings"])
            t = clock(lambda: bm.update(which, which, lens, off, terms, tfs, docs, vocab, total, docs))
            if i >= WARMUP:
                ms.append(t)
        off, terms, tfs = batches[-1]
        ctx.profile_enable(True)
        bm.update(which, which, lens, off, terms, tfs, docs, vocab, total, docs)
        stages = {name: round(ctx.profile_read("bm25_update_" + name)[1], 3) for name in ("live", "order", "offsets", "merge")}
        ctx.profile_enable(False)
        n_new = bm.stats()["postings"]
        streamed = 12 * int(np.median(n_old)) + 8 * n_new + 24 * int(terms.size) * radix_passes(docs, vocab)
        t0 = time.perf_counter()
        term_off, post_doc, post_tf = assemble(term_off, post_doc, post_tf, vocab, which, off, terms, tfs)
        assemble_ms = (time.perf_counter() - t0) * 1e3
        got = bm.export()
        assert np.array_equal(got[0], term_off) and np.array_equal(got[1], post_doc) and np.array_equal(got[2], post_tf) and \
            np.array_equal(got[3], doc_len), f"B = {b}: the updated image is not the host's"
        del got
        create_ms = []
        for _ in range(CREATE_REPS):
            def recreate():
                nonlocal other
                if other is not None:
                    other.close()
                other = vg.Bm25(ctx, term_off, post_doc, post_tf, doc_len, total, docs)
            create_ms.append(clock(recreate))
        u, c = spread(ms), spread(create_ms)
        report["batches"][str(b)] = {
            "added_postings": int(terms.size), "update_ms": u, "stage_ms": stages, "streamed_bytes": streamed,
            "update_gbs": round(streamed / (u["median"] * 1e-3) / 1e9, 1), "stream_fraction": round(streamed / (u["median"] * 1e-3) / (STREAM_TBS * 1e12), 4),
            "recreate_ms": c, "assemble_ms": round(assemble_ms, 1), "ratio_call": round(c["median"] / u["median"], 2),
            "ratio_with_assembly": round((assemble_ms + c["median"]) / u["median"], 2)}
        print(b, report["batches"][str(b)], flush=True)
    report["resident_bytes"] = bm.stats()["bytes"]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
