"""The three promises of include/vecgo_hip.h for device-resident callers, entry by entry, against the CPU oracle:

  A  any element-aligned device pointer gives the same bits as an aligned one: every caller buffer (inputs, and outputs
     through out= where the API has it) as a view one element past a larger allocation.  Call sites that test the pointer
     (aligned16) then launch their element kernels at shapes that normally take the 16-byte ones; everywhere else the
     library stages the view through a scratch block (vg::Align, vg_internal.hpp).
  B  a call on a caller's stream is ordered on that stream and on nothing else: the inputs are still poison (NaN / 0xFF) when
     the call is made — their producer sits behind a 20 .. 60 ms delay on a fresh non-blocking stream —, and are poisoned
     again right behind the call.  Entries that only enqueue return before the producer has finished (asserted for the
     list in the header).  Two streams, back to back and from two threads, must not share per-call scratch.
  C  host and device buffers mixed in one call.
"""
import threading

import numpy as np
import pytest

from oracle import oracle as o
from tests import graphs, hooks
from tests.threshold_ref import engine_filter

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
N_CODEC = 2053    # rows of the codec cases: odd, 129 row-walk blocks of 16
N_FLAT = 6000     # rows of the flat-family cases (a multiple of 8: a 0xFF mask names no row past the end)
N_GRAPH = 2000    # nodes of the walks
K = 10

# every vg::ProfScope name a case may see (profile records are per name)
SCOPES = ("pq_encode", "pq_build_table", "int4_scan", "km_assign", "flat_scan", "flat_gemm", "flat_select", "flat_probe",
          "flat_probe_gemm", "flat_thr_scan", "flat_thr_gemm", "flat_thr_select", "flat_thr_rescore", "sq8_scan", "sq8_probe",
          "sq8_nominate_gemm", "pq_adc_scan", "pq_adc_probe", "rabitq_scan", "rabitq_scan_mq", "hnsw_search_pq", "hnsw_predicate",
          "hnsw_brute_dist", "hnsw_brute_replay", "vamana_search", "rerank")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def db(torch):
    from tests import devbuf
    return devbuf


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


class Ragged:
    """per-query result lists that may be shorter than k: the first len(rows[q]) entries of row q, and for ids the padding"""

    def __init__(self, rows, pad_invalid=False):
        self.rows, self.pad_invalid = rows, pad_invalid


class Case:
    """One entry point at one shape.  ins: the caller's input buffers (numpy); outs: (shape, dtype) of the buffers the API
    takes through out= (none: the API allocates them next to the inputs); call(b, out, stream) -> tuple of results; want: the
    oracle's, one per result; prof: ProfScope names that must have launched; poison: what late inputs hold instead of 0xFF /
    NaN where garbage must stay a valid index (a PQ code below k, a candidate id below n); inout: an input that is also the
    first result (normalize_l2); host_results: some results are host arrays whatever the inputs (per-query stats)."""

    def __init__(self, ins, call, want, outs=(), prof=(), poison=None, inout=None, host_results=False):
        self.ins, self.call, self.want, self.outs = ins, call, want, tuple(outs)
        self.prof, self.poison, self.inout, self.host_results = tuple(prof), poison or {}, inout, host_results


def _first(out):
    return None if out is None else out[0]


def _rows(fn, n):
    return np.stack([fn(i) for i in range(n)])


def _packed(mask):
    return np.packbits(mask, axis=-1, bitorder="little")


class World:
    """Every quantizer, index and oracle answer of this file, built once per family and left unchanged."""

    def __init__(self, vg, ctx):
        self.vg, self.ctx = vg, ctx
        self.cases = {}
        self._built = set()

    def __getitem__(self, name):
        fam = FAMILY_OF[name]
        if fam not in self._built:
            made = getattr(self, "_build_" + fam)()
            assert sorted(made) == sorted(n for n, f in FAMILY_OF.items() if f == fam), (fam, sorted(made))
            self.cases.update(made)
            self._built.add(fam)
        return self.cases[name]

    # ---- codecs --------------------------------------------------------------------------------------------------
    def _build_sq8(self):
        vg, ctx, out, n = self.vg, self.ctx, {}, N_CODEC
        for dim in (128, 100):
            rng = np.random.default_rng(1000 + dim)
            x = rng.standard_normal((n, dim)).astype(np.float32)
            ref = o.ScalarQuantizer(dim); ref.train(x)
            sq = vg.ScalarQuantizer(ctx, dim); sq.train(x)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                       for a, b in zip(sq.params(), (ref.mins, ref.maxs, ref.scales, ref.inv_scales)))
            for tag, rows in (("", x * 1.5), ("@2", x[::-1] * 0.5)):   # * 1.5: values to clamp
                rows = np.ascontiguousarray(rows, np.float32)
                if tag and dim != 128:
                    continue
                out[f"sq8_encode[{dim}]{tag}"] = Case({"v": rows}, lambda b, out_, s, sq=sq: (sq.encode(b["v"], out=_first(out_), stream=s),),
                                                      (ref.encode_batch(rows),), outs=[((n, dim), np.uint8)])
            codes = ref.encode_batch(x)
            out[f"sq8_decode[{dim}]"] = Case({"c": codes}, lambda b, out_, s, sq=sq: (sq.decode(b["c"], out=_first(out_), stream=s),),
                                             (_rows(lambda i: ref.decode(codes[i]), n),), outs=[((n, dim), np.float32)])
            q = rng.standard_normal(dim).astype(np.float32)
            out[f"sq8_l2[{dim}]"] = Case({"q": q, "c": codes},
                                         lambda b, out_, s, sq=sq: (sq.l2_distance_batch(b["q"], b["c"], out=_first(out_), stream=s),),
                                         (o.sq8u_l2_batch(q, codes, ref.mins, ref.inv_scales, dim),), outs=[((n,), np.float32)])
        return out

    def _build_int4(self):
        vg, ctx, out, n, dim = self.vg, self.ctx, {}, N_CODEC, 128
        rng = np.random.default_rng(2000)
        x = (rng.standard_normal((n, dim)) * rng.random(dim) * 3).astype(np.float32)
        ref = o.Int4Quantizer(dim); ref.train(x)
        iq = vg.Int4Quantizer(ctx, dim); iq.train(x)
        mn, df, _ = iq.params()
        assert np.array_equal(mn.view(np.uint32), ref.min.view(np.uint32)) and np.array_equal(df.view(np.uint32), ref.diff.view(np.uint32))
        y = np.ascontiguousarray(x * 1.5, np.float32)
        codes = ref.encode_batch(x)
        q = (rng.standard_normal(dim) * 2).astype(np.float32)
        cb = (dim + 1) // 2
        out["int4_encode[128]"] = Case({"v": y}, lambda b, out_, s: (iq.encode(b["v"], out=_first(out_), stream=s),),
                                       (ref.encode_batch(y),), outs=[((n, cb), np.uint8)])
        out["int4_decode[128]"] = Case({"c": codes}, lambda b, out_, s: (iq.decode(b["c"], out=_first(out_), stream=s),),
                                       (_rows(lambda i: ref.decode(codes[i]), n),), outs=[((n, dim), np.float32)])
        out["int4_l2_distance[128]"] = Case({"q": q, "c": codes}, lambda b, out_, s: (iq.l2_distance(b["q"], b["c"], out=_first(out_), stream=s),),
                                            (np.array([ref.l2_distance(q, c) for c in codes], np.float32),), outs=[((n,), np.float32)],
                                            prof=("int4_scan",))
        out["int4_l2_distance_batch[128]"] = Case({"q": q, "c": codes},
                                                  lambda b, out_, s: (iq.l2_distance_batch(b["q"], b["c"], out=_first(out_), stream=s),),
                                                  (ref.l2_distance_batch(q, codes),), outs=[((n,), np.float32)], prof=("int4_scan",))
        return out

    def _random_pq(self, rng, dim, m, k):
        sd = dim // m
        ref = o.ProductQuantizer(dim, m, k)
        ref.set_codebooks(rng.integers(-128, 128, m * k * sd).astype(np.int8), (rng.random(m) * 0.02 + 0.005).astype(np.float32),
                          ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32))
        pq = self.vg.ProductQuantizer(self.ctx, dim, m, k)
        pq.set_codebooks(ref.codebooks, ref.scales, ref.offsets)
        return ref, pq

    def _build_pq(self):
        vg, ctx, out, n = self.vg, self.ctx, {}, N_CODEC
        for dim, m, k in ((768, 96, 256), (64, 16, 64), (128, 8, 256)):
            rng = np.random.default_rng(3000 + dim)
            ref, pq = self._random_pq(rng, dim, m, k)
            t = f"[{dim},{m},{k}]"
            x = rng.standard_normal((n, dim)).astype(np.float32)
            codes = ref.encode_batch(x)
            code_poison = {"c": k - 1} if k < 256 else None   # a late code must stay below k
            out["pq_encode" + t] = Case({"v": x}, lambda b, out_, s, pq=pq: (pq.encode(b["v"], out=_first(out_), stream=s),), (codes,),
                                        outs=[((n, m), np.uint8)], prof=("pq_encode",))
            out["pq_decode" + t] = Case({"c": codes}, lambda b, out_, s, pq=pq: (pq.decode(b["c"], out=_first(out_), stream=s),),
                                        (_rows(lambda i: ref.decode(codes[i]), n),), outs=[((n, dim), np.float32)], poison=code_poison)
            for tag, seed in (("", 1), ("@2", 2)):
                if tag and dim != 768:
                    continue
                q = np.random.default_rng(3100 + dim + seed).standard_normal(dim).astype(np.float32)
                out["pq_asym" + t + tag] = Case({"q": q, "c": codes},
                                                lambda b, out_, s, pq=pq: (pq.asymmetric_distance(b["q"], b["c"], out=_first(out_), stream=s),),
                                                (np.array([ref.asym_distance(q, c) for c in codes], np.float32),), outs=[((n,), np.float32)],
                                                poison=code_poison)
            qs = rng.standard_normal((5, dim)).astype(np.float32)
            out["pq_table" + t] = Case({"q": qs}, lambda b, out_, s, pq=pq: (pq.build_distance_table(b["q"], out=_first(out_), stream=s),),
                                       (_rows(lambda i: ref.build_table(qs[i]), 5),), outs=[((5, m * k), np.float32)], prof=("pq_build_table",))
            if k == 256:   # simd.PqAdcLookup reads 256 entries per sub-quantizer
                table = ref.build_table(qs[0])
                out["pq_adc_lookup" + t] = Case({"t": table, "c": codes},
                                                lambda b, out_, s, m=m: (vg.pq_adc_lookup_batch(ctx, b["t"], b["c"], m, stream=s),),
                                                (np.array([o.adc(table, c, m) for c in codes], np.float32),))
        return out

    def _build_opq(self):
        vg, ctx, out, n = self.vg, self.ctx, {}, N_CODEC
        for dim, m, k in ((128, 16, 64), (64, 8, 16)):
            rng = np.random.default_rng(4000 + dim)
            ref = o.OptimizedProductQuantizer(dim, m, k)   # rotation blocks (vg_opq_block_size): 32 at (128, 16), 64 at (64, 8)
            rot = np.stack([np.linalg.qr(rng.standard_normal((ref.block, ref.block)))[0] for _ in range(ref.nblocks)]).astype(np.float32)
            sd = dim // m
            cb = rng.integers(-128, 128, m * k * sd).astype(np.int8)
            sc, of = (rng.random(m) * 0.02 + 0.005).astype(np.float32), ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32)
            ref.rotations = rot; ref.pq.set_codebooks(cb, sc, of)
            opq = vg.OptimizedProductQuantizer(ctx, dim, m, k)
            assert opq.block == ref.block and opq.nblocks == ref.nblocks
            opq.set_rotations(rot); opq.pq.set_codebooks(cb, sc, of)
            t = f"[{dim},{m},{k}]"
            x = rng.standard_normal((n, dim)).astype(np.float32)
            codes = _rows(lambda i: ref.encode(x[i]), n)
            q = rng.standard_normal(dim).astype(np.float32)
            out["opq_rotate" + t] = Case({"v": x}, lambda b, out_, s, opq=opq: (opq.rotate(b["v"], out=_first(out_), stream=s),),
                                         (_rows(lambda i: ref.rotate(x[i]), n),), outs=[((n, dim), np.float32)])
            out["opq_encode" + t] = Case({"v": x}, lambda b, out_, s, opq=opq: (opq.encode(b["v"], out=_first(out_), stream=s),), (codes,),
                                         outs=[((n, m), np.uint8)], prof=("pq_encode",))
            out["opq_decode" + t] = Case({"c": codes}, lambda b, out_, s, opq=opq: (opq.decode(b["c"], out=_first(out_), stream=s),),
                                         (_rows(lambda i: ref.decode(codes[i]), n),), outs=[((n, dim), np.float32)], poison={"c": k - 1})
            out["opq_asym" + t] = Case({"q": q, "c": codes},
                                       lambda b, out_, s, opq=opq: (opq.asymmetric_distance(b["q"], b["c"], out=_first(out_), stream=s),),
                                       (np.array([ref.asym_distance(q, c) for c in codes], np.float32),), outs=[((n,), np.float32)],
                                       poison={"c": k - 1})
        return out

    def _build_binary(self):
        vg, ctx, out, n = self.vg, self.ctx, {}, N_CODEC
        for dim in (128, 100):
            rng = np.random.default_rng(5000 + dim)
            x = (rng.standard_normal((n, dim)) * 2 + 0.3).astype(np.float32)
            x[3] = 0.0    # zero norm: reported, left untouched
            th = 0.3
            bq = vg.BinaryQuantizer(ctx, dim).with_threshold(th)
            nb = bq.words * 8
            codes = _rows(lambda i: o.binary_encode_u64(x[i], th).view(np.uint8), n)
            q = rng.standard_normal(dim).astype(np.float32)
            qc = o.binary_encode_u64(q, th).view(np.uint8)
            out[f"binary_encode[{dim}]"] = Case({"v": x}, lambda b, out_, s, bq=bq: (bq.encode(b["v"], out=_first(out_), stream=s),), (codes,),
                                                outs=[((n, nb), np.uint8)])
            out[f"binary_decode[{dim}]"] = Case({"c": codes}, lambda b, out_, s, bq=bq: (bq.decode(b["c"], out=_first(out_), stream=s),),
                                                (_rows(lambda i: o.binary_decode(codes[i], dim, th), n),), outs=[((n, dim), np.float32)])
            out[f"binary_hamming[{dim}]"] = Case({"q": q, "c": codes},
                                                 lambda b, out_, s, bq=bq: (bq.compute_hamming_distance(b["q"], b["c"], out=_first(out_), stream=s),),
                                                 (np.array([o.hamming(qc, c) for c in codes], np.int32),), outs=[((n,), np.int32)])
            norm = [o.normalize_l2(x[i]) for i in range(n)]

            def normalize(b, out_, s, dim=dim):
                ok = vg.normalize_l2(ctx, b["v"], dim, stream=s)
                return b["v"], ok
            out[f"normalize_l2[{dim}]"] = Case({"v": x}, normalize, (np.stack([v for v, _ in norm]), np.array([ok for _, ok in norm], np.uint8)),
                                               inout="v")
        return out

    def _build_rabitq(self):
        vg, ctx, out, n, dim = self.vg, self.ctx, {}, N_CODEC, 128
        rng = np.random.default_rng(6000)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        rq = vg.RaBitQuantizer(ctx, dim)
        codes = o.rabitq_encode_batch(x, dim)
        q = rng.standard_normal(dim).astype(np.float32)
        out["rabitq_encode[128]"] = Case({"v": x}, lambda b, out_, s: (rq.encode(b["v"], out=_first(out_), stream=s),), (codes,),
                                         outs=[((n, rq.bytes_total()), np.uint8)])
        out["rabitq_distance[128]"] = Case({"q": q, "c": codes}, lambda b, out_, s: (rq.distance(b["q"], b["c"], out=_first(out_), stream=s),),
                                           (np.array([o.rabitq_distance(q, c) for c in codes], np.float32),), outs=[((n,), np.float32)])
        return out

    def _build_kmeans(self):
        vg, ctx, out, dim, k = self.vg, self.ctx, {}, 128, 12
        for n in (N_CODEC, 4500):    # 4500: enough points for the matrix-core nomination (KmMfma::eligible)
            rng = np.random.default_rng(7000 + n)
            x = rng.standard_normal((n, dim)).astype(np.float32)
            cent = rng.standard_normal((k, dim)).astype(np.float32)
            want = np.array([o.assign_partition(x[i], cent, dim, 0) for i in range(n)], np.int32)
            out[f"kmeans_assign[{n}x128]"] = Case({"v": x, "c": cent},
                                                  lambda b, out_, s: (vg.kmeans_assign(ctx, b["v"], b["c"], dim, 0, stream=s),), (want,),
                                                  prof=("km_assign",))
        return out

    # ---- the flat family -----------------------------------------------------------------------------------------
    def _build_flat(self):
        vg, ctx, out, n = self.vg, self.ctx, {}, N_FLAT
        ids_sc = lambda nq, k=K: [((nq, k), np.uint32), ((nq, k), np.float32)]
        for dim in (128, 100):
            rng = np.random.default_rng(8000 + dim)
            base = rng.standard_normal((n, dim)).astype(np.float32)
            base[37] = base[12]    # a tie: broken by the row id
            idx = vg.Index(ctx, n, dim)
            idx.set_vectors(base)
            seg = o.FlatSegment(base, dim)

            def flat_want(q, k=K):
                r = [o.flat_search_f32(base, dim, q[i], k) for i in range(q.shape[0])]
                assert all(e[0].size == k for e in r)
                return np.stack([e[0] for e in r]), np.stack([e[1] for e in r])
            for nq in ((1, 8, 200) if dim == 128 else (8,)):
                for tag, seed in (("", 0), ("@2", 1)):
                    if tag and nq != 200:
                        continue
                    q = np.random.default_rng(8100 + dim + nq + seed).standard_normal((nq, dim)).astype(np.float32)
                    q[0] = base[12] + 0.001
                    out[f"search_flat[{dim},nq{nq}]{tag}"] = Case({"q": q}, lambda b, out_, s, idx=idx: idx.search_flat(b["q"], K, out=out_, stream=s),
                                                                  flat_want(q), outs=ids_sc(nq), prof=("flat_scan",) if nq == 1 else ("flat_gemm",))
            q = rng.standard_normal((8, dim)).astype(np.float32)
            # thresholds: each query's 6th-best distance, so 6 of max_results = 16 rows are within it (one query keeps none)
            fid, fsc = flat_want(q, 16)
            thr = fsc[:, 5].copy(); thr[3] = 0.0
            filt = [engine_filter(fid[i], fsc[i], thr[i], False, 16) for i in range(8)]
            out[f"search_flat_threshold[{dim}]"] = Case(
                {"q": q, "t": thr}, lambda b, out_, s, idx=idx: idx.search_flat_threshold(b["q"], b["t"], 16, out=out_, stream=s),
                (np.stack([f[0] for f in filt]), np.stack([f[1] for f in filt]), np.array([f[2] for f in filt], np.int32)),
                outs=[((8, 16), np.uint32), ((8, 16), np.float32), ((8,), np.int32)], prof=("flat_thr_scan", "flat_thr_select"))
            mask = rng.random((8, n)) < 0.3
            fw = [seg.search(q[i], K, mask=mask[i]) for i in range(8)]
            assert all(e[0].size == K for e in fw)
            out[f"search_flat_filtered[{dim}]"] = Case(
                {"q": q, "m": _packed(mask)}, lambda b, out_, s, idx=idx: idx.search_flat_filtered(b["q"], K, b["m"], 0, out=out_, stream=s),
                (np.stack([e[0] for e in fw]), np.stack([e[1] for e in fw])), outs=ids_sc(8), prof=("flat_gemm",))
        return out

    def _build_probed(self):
        vg, ctx, out, n, dim, parts, nprobes = self.vg, self.ctx, {}, N_FLAT, 128, 7, 3
        rng = np.random.default_rng(9000)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        cent = (rng.standard_normal((parts, dim)) * 0.7).astype(np.float32)
        a = np.array([o.assign_partition(x[i], cent, dim, 0) for i in range(n)], np.int64)
        order = np.argsort(a, kind="stable")
        x, a = np.ascontiguousarray(x[order]), a[order]
        off = np.searchsorted(a, np.arange(parts + 1)).astype(np.uint32)
        osq = o.ScalarQuantizer(dim); osq.train(x)
        sq = vg.ScalarQuantizer(ctx, dim); sq.train(x)
        sq_codes = osq.encode_batch(x)
        opq, pq = self._random_pq(rng, dim, 16, 256)
        pq_codes = opq.encode_batch(x)
        idx = vg.Index(ctx, n, dim)
        idx.set_vectors(x); idx.set_sq8_codes(sq, sq_codes); idx.set_pq_codes(pq, pq_codes); idx.set_partitions(cent, off)
        self._probed_keep = (idx, sq, pq)
        segs = {idx.SCAN_F32: o.FlatSegment(x, dim, centroids=cent, part_offsets=off),
                idx.SCAN_SQ8: o.FlatSegment(x, dim, sq=osq, codes=sq_codes, centroids=cent, part_offsets=off),
                idx.SCAN_PQ: o.FlatSegment(x, dim, pq=opq, codes=pq_codes, centroids=cent, part_offsets=off)}
        for name, scan, nq, prof in (("f32,nq9", idx.SCAN_F32, 9, ("flat_probe",)), ("f32,nq200", idx.SCAN_F32, 200, ("flat_probe", "flat_probe_gemm")),
                                     ("sq8,nq9", idx.SCAN_SQ8, 9, ("sq8_probe",)), ("pq,nq9", idx.SCAN_PQ, 9, ("pq_adc_probe",))):
            q = np.random.default_rng(9100 + nq + scan).standard_normal((nq, dim)).astype(np.float32)
            w = [segs[scan].search(q[i], K, nprobes) for i in range(nq)]
            assert all(e[0].size == K for e in w)
            out[f"search_flat_probed[{name}]"] = Case(
                {"q": q}, lambda b, out_, s, scan=scan: idx.search_flat_probed(b["q"], K, nprobes, scan, out=out_, stream=s),
                (np.stack([e[0] for e in w]), np.stack([e[1] for e in w])), outs=[((nq, K), np.uint32), ((nq, K), np.float32)], prof=prof)
        return out

    def _build_scans(self):
        vg, ctx, out, n = self.vg, self.ctx, {}, N_FLAT
        ids_sc = lambda nq: [((nq, K), np.uint32), ((nq, K), np.float32)]
        # SQ8 with the bf16 nomination switched on: 4 queries keep the scan, 6 take the nomination (VG_SQ8_NOM_MIN_Q = 5)
        dim = 128
        rng = np.random.default_rng(10000)
        x = rng.standard_normal((n, dim)).astype(np.float32)
        x[37] = x[12]
        osq = o.ScalarQuantizer(dim); osq.train(x)
        sq = vg.ScalarQuantizer(ctx, dim); sq.train(x)
        codes = osq.encode_batch(x)
        sidx = vg.Index(ctx, n, dim)
        sidx.set_sq8_codes(sq, codes)
        sidx.enable_sq8_nomination(True)
        for nq, tag, seed in ((4, "", 0), (6, "", 0), (6, "@2", 1)):
            q = np.random.default_rng(10100 + nq + seed).standard_normal((nq, dim)).astype(np.float32)
            q[0] = x[12] + 0.001
            w = [o.flat_search_sq8(osq, codes, q[i], K) for i in range(nq)]
            out[f"search_sq8[nom,nq{nq}]{tag}"] = Case({"q": q}, lambda b, out_, s: sidx.search_sq8(b["q"], K, out=out_, stream=s),
                                                       (np.stack([e[0] for e in w]), np.stack([e[1] for e in w])), outs=ids_sc(nq),
                                                       prof=("sq8_nominate_gemm",) if nq >= 5 else ("sq8_scan",))
        # RaBitQ
        rcodes = o.rabitq_encode_batch(x, dim)
        ridx = vg.Index(ctx, n, dim)
        ridx.set_rabitq_codes(rcodes)
        q = rng.standard_normal((4, dim)).astype(np.float32)
        w = [o.flat_search_rabitq(rcodes, dim, q[i], K) for i in range(4)]
        out["search_rabitq[nq4]"] = Case({"q": q}, lambda b, out_, s: ridx.search_rabitq(b["q"], K, out=out_, stream=s),
                                         (np.stack([e[0] for e in w]), np.stack([e[1] for e in w])), outs=ids_sc(4), prof=("rabitq_scan_mq",))
        # PQ-ADC with the nomination over the decoded rows forced for a small batch (VG_PQ_NOM_ALWAYS)
        dim, m = 768, 96
        rng = np.random.default_rng(10200)
        xp = rng.standard_normal((n, dim)).astype(np.float32)
        opq, pq = self._random_pq(rng, dim, m, 256)
        pcodes = opq.encode_batch(xp)
        pidx = vg.Index(ctx, n, dim)
        pidx.set_pq_codes(pq, pcodes)
        pidx.enable_pq_nomination(True)
        qp = rng.standard_normal((8, dim)).astype(np.float32)
        w = [o.flat_search_pq(opq, pcodes, qp[i], K) for i in range(8)]

        def pq_nominated(b, out_, s):
            hooks.set_hook("VG_PQ_NOM_ALWAYS", 1)
            try:
                return pidx.search_pq_adc(b["q"], K, out=out_, stream=s)
            finally:
                hooks.set_hook("VG_PQ_NOM_ALWAYS", 0)
        out["search_pq_adc[nom,nq8]"] = Case({"q": qp}, pq_nominated, (np.stack([e[0] for e in w]), np.stack([e[1] for e in w])), outs=ids_sc(8),
                                             prof=("sq8_nominate_gemm",))   # the nomination GEMM both quantizers share
        self._scans_keep = (sq, pq)
        return out

    # ---- walks and helpers ---------------------------------------------------------------------------------------
    def _build_walks(self):
        vg, ctx, out, n, nq, ef = self.vg, self.ctx, {}, N_GRAPH, 8, 64

        def ragged(res):
            return Ragged([r[0] for r in res], pad_invalid=True), Ragged([r[1] for r in res])

        def stats4(res):
            return np.array([[r[2].nodes_visited, r[2].distance_computations, r[2].distance_short_circuits, r[2].pops] for r in res], np.int64)

        def with_stats(ins, call_stats, want, res, cols=None):
            """the same walk with stats=True: a host array of counters beside the device (or skewed) ids, scores, masks and
            thresholds of one call; cols: the counters the oracle has for this walk (Vamana: no short-circuit counter)"""
            pick = (lambda st: np.ascontiguousarray(st)) if cols is None else (lambda st: np.ascontiguousarray(st[:, cols]))

            def call(b, out_, s):
                r = call_stats(b, s)
                return tuple(r[:-1]) + (pick(r[-1]),)
            return Case(ins, call, tuple(want) + (pick(stats4(res)),), host_results=True)
        V = [0, 1, 3]   # nodes_visited, distance_computations, pops
        for dim in (32, 768):
            rng = np.random.default_rng(11000 + dim)
            base = rng.standard_normal((n, dim)).astype(np.float32)
            l0, upper, entry = graphs.build_hnsw(base, m=8, seed=dim)
            g, ventry = graphs.build_vamana(base, r=16, seed=dim)
            pm = dim // 8
            opq, pq = self._random_pq(rng, dim, pm, 256)
            pcodes = opq.encode_batch(base)
            rcodes = o.rabitq_encode_batch(base, dim)
            oiq = o.Int4Quantizer(dim); oiq.train(base)
            iq = vg.Int4Quantizer(ctx, dim); iq.train(base)
            icodes = oiq.encode_batch(base)
            idx = vg.Index(ctx, n, dim)
            idx.set_vectors(base); idx.set_hnsw_graph(l0, upper, entry, m=8); idx.set_vamana_graph(g, ventry)
            idx.set_pq_codes(pq, pcodes); idx.set_rabitq_codes(rcodes); idx.set_int4_codes(iq, icodes)
            self.__dict__.setdefault("_walk_keep", []).append((idx, pq, iq))
            oh = o.HnswIndex(base, dim, l0, upper, entry, m=8)
            ohp = o.HnswIndex(base, dim, l0, upper, entry, m=8, pq=opq, codes=pcodes)
            t = f"[{dim}]"
            for tag, seed in (("", 0), ("@2", 1)):
                q = np.random.default_rng(11100 + dim + seed).standard_normal((nq, dim)).astype(np.float32)
                res = [oh.search(q[i], K, ef) for i in range(nq)]
                out["search_hnsw" + t + tag] = Case({"q": q}, lambda b, out_, s, idx=idx: idx.search_hnsw(b["q"], K, ef, stream=s), ragged(res))
                if not tag:
                    out["search_hnsw_stats" + t] = Case({"q": q}, lambda b, out_, s, idx=idx: idx.search_hnsw(b["q"], K, ef, stats=True, stream=s),
                                                        ragged(res) + (stats4(res),), host_results=True)
                ov = o.VamanaIndex(g, ventry, dim, o.VAMANA_F32, base=base)
                res = [ov.search(q[i], K) for i in range(nq)]
                out["search_vamana[0]" + t + tag] = Case({"q": q}, lambda b, out_, s, idx=idx: idx.search_vamana(b["q"], K, kind=0, stream=s),
                                                         ragged(res), prof=("vamana_search",))
            res = [ohp.search(q[i], K, ef) for i in range(nq)]
            out["search_hnsw_pq" + t] = Case({"q": q}, lambda b, out_, s, idx=idx: idx.search_hnsw_pq(b["q"], K, ef, stream=s), ragged(res),
                                             prof=("hnsw_search_pq",))
            out["search_hnsw_pq_stats" + t] = with_stats({"q": q}, lambda b, s, idx=idx: idx.search_hnsw_pq(b["q"], K, ef, stats=True, stream=s),
                                                         ragged(res), res)
            mask = rng.random((nq, n)) < 0.5
            res = [oh.search_filtered(q[i], K, ef, mask[i], 0.5) for i in range(nq)]
            out["search_hnsw_filtered" + t] = Case({"q": q, "m": _packed(mask)},
                                                   lambda b, out_, s, idx=idx: idx.search_hnsw_filtered(b["q"], K, ef, b["m"], 0.5, stream=s),
                                                   ragged(res))
            out["search_hnsw_filtered_stats" + t] = with_stats(
                {"q": q, "m": _packed(mask)}, lambda b, s, idx=idx: idx.search_hnsw_filtered(b["q"], K, ef, b["m"], 0.5, stats=True, stream=s),
                ragged(res), res)
            pmask = rng.random((nq, n)) < 0.2
            res = [oh.search_predicate(q[i], K, ef, pmask[i]) for i in range(nq)]
            out["search_hnsw_predicate" + t] = Case({"q": q, "m": _packed(pmask)},
                                                    lambda b, out_, s, idx=idx: idx.search_hnsw_predicate(b["q"], K, ef, b["m"], stream=s),
                                                    ragged(res), prof=("hnsw_predicate",))
            out["search_hnsw_predicate_stats" + t] = with_stats(
                {"q": q, "m": _packed(pmask)}, lambda b, s, idx=idx: idx.search_hnsw_predicate(b["q"], K, ef, b["m"], stats=True, stream=s),
                ragged(res), res)
            member = rng.random(n) < 0.3
            for mode in (0, 1):
                res = [oh.brute_search(q[i], K, mode, member) for i in range(nq)]
                out[f"search_hnsw_brute[{mode}]" + t] = Case(
                    {"q": q, "m": _packed(member)}, lambda b, out_, s, idx=idx, mode=mode: idx.search_hnsw_brute(b["q"], K, mode, b["m"], stream=s),
                    ragged(res), prof=("hnsw_brute_dist",))
            for kind, ov in ((1, o.VamanaIndex(g, ventry, dim, o.VAMANA_PQ, pq=opq, codes=pcodes)),
                             (2, o.VamanaIndex(g, ventry, dim, o.VAMANA_RABITQ, codes=rcodes)),
                             (3, o.VamanaIndex(g, ventry, dim, o.VAMANA_INT4, codes=icodes, int4_table=oiq.table))):
                res = [ov.search(q[i], K) for i in range(nq)]
                out[f"search_vamana[{kind}]" + t] = Case({"q": q}, lambda b, out_, s, idx=idx, kind=kind: idx.search_vamana(b["q"], K, kind=kind, stream=s),
                                                         ragged(res), prof=("vamana_search",))
                out[f"search_vamana_stats[{kind}]" + t] = with_stats(
                    {"q": q}, lambda b, s, idx=idx, kind=kind: idx.search_vamana(b["q"], K, kind=kind, stats=True, stream=s), ragged(res), res, V)
            ov = o.VamanaIndex(g, ventry, dim, o.VAMANA_F32, base=base)
            res = [ov.search(q[i], K) for i in range(nq)]

            def vamana_stats(b, out_, s, idx=idx):   # (the walk has no short-circuit counter: column 2 is not the oracle's)
                ids, sc, st = idx.search_vamana(b["q"], K, kind=0, stats=True, stream=s)
                return ids, sc, np.ascontiguousarray(st[:, [0, 1, 3]])
            out["search_vamana_stats" + t] = Case({"q": q}, vamana_stats, ragged(res) + (np.ascontiguousarray(stats4(res)[:, [0, 1, 3]]),),
                                                  host_results=True)
            vmask = rng.random((nq, n)) < 0.5
            res = [ov.search(q[i], K, mask=vmask[i]) for i in range(nq)]
            out["search_vamana_filtered" + t] = Case({"q": q, "m": _packed(vmask)},
                                                     lambda b, out_, s, idx=idx: idx.search_vamana_filtered(b["q"], K, b["m"], kind=0, stream=s),
                                                     ragged(res))
            out["search_vamana_filtered_stats" + t] = with_stats(
                {"q": q, "m": _packed(vmask)}, lambda b, s, idx=idx: idx.search_vamana_filtered(b["q"], K, b["m"], kind=0, stats=True, stream=s),
                ragged(res), res, V)
            # threshold walk: the 16-result walk, then the rows within each query's 5th-best distance
            res = [ov.search(q[i], 16) for i in range(nq)]
            thr = np.array([r[1][4] for r in res], np.float32)
            filt = [engine_filter(res[i][0], res[i][1], thr[i], False, 16) for i in range(nq)]
            out["search_vamana_threshold" + t] = Case(
                {"q": q, "t": thr}, lambda b, out_, s, idx=idx: idx.search_vamana_threshold(b["q"], b["t"], 16, kind=0, stream=s),
                (np.stack([f[0] for f in filt]), np.stack([f[1] for f in filt]), np.array([f[2] for f in filt], np.int32)))
            out["search_vamana_threshold_stats" + t] = with_stats(
                {"q": q, "t": thr}, lambda b, s, idx=idx: idx.search_vamana_threshold(b["q"], b["t"], 16, kind=0, stats=True, stream=s),
                out["search_vamana_threshold" + t].want, res, V)
            cand = np.stack([rng.choice(n, 40, replace=False) for _ in range(nq)]).astype(np.uint32)
            exact = _rows(lambda i: o.rerank_f32(base, dim, q[i], cand[i]), nq)
            order = [np.lexsort((cand[i], exact[i]))[:K] for i in range(nq)]
            out["rerank" + t] = Case({"q": q, "cand": cand}, lambda b, out_, s, idx=idx: idx.rerank(b["q"], b["cand"], K, out=out_, stream=s),
                                     (_rows(lambda i: cand[i][order[i]], nq), _rows(lambda i: exact[i][order[i]], nq)),
                                     outs=[((nq, K), np.uint32), ((nq, K), np.float32)], poison={"cand": 0}, prof=("rerank",))
            out["score_candidates" + t] = Case({"q": q, "cand": cand},
                                               lambda b, out_, s, idx=idx: (idx.score_candidates(b["q"], b["cand"], out=_first(out_), stream=s),),
                                               (exact,), outs=[((nq, 40), np.float32)], poison={"cand": 0})
        return out


def _names():
    f = {}
    for dim in (128, 100):
        for e in ("sq8_encode", "sq8_decode", "sq8_l2"):
            f[f"{e}[{dim}]"] = "sq8"
        for e in ("binary_encode", "binary_decode", "binary_hamming", "normalize_l2"):
            f[f"{e}[{dim}]"] = "binary"
        f[f"search_flat_threshold[{dim}]"] = f[f"search_flat_filtered[{dim}]"] = "flat"
    f["sq8_encode[128]@2"] = "sq8"
    for e in ("int4_encode", "int4_decode", "int4_l2_distance", "int4_l2_distance_batch"):
        f[e + "[128]"] = "int4"
    for dim, m, k in ((768, 96, 256), (64, 16, 64), (128, 8, 256)):
        for e in ("pq_encode", "pq_decode", "pq_asym", "pq_table") + (("pq_adc_lookup",) if k == 256 else ()):
            f[f"{e}[{dim},{m},{k}]"] = "pq"
    f["pq_asym[768,96,256]@2"] = "pq"
    for dim, m, k in ((128, 16, 64), (64, 8, 16)):
        for e in ("opq_rotate", "opq_encode", "opq_decode", "opq_asym"):
            f[f"{e}[{dim},{m},{k}]"] = "opq"
    f["rabitq_encode[128]"] = f["rabitq_distance[128]"] = "rabitq"
    f[f"kmeans_assign[{N_CODEC}x128]"] = f["kmeans_assign[4500x128]"] = "kmeans"
    for nq in (1, 8, 200):
        f[f"search_flat[128,nq{nq}]"] = "flat"
    f["search_flat[128,nq200]@2"] = f["search_flat[100,nq8]"] = "flat"
    for t in ("f32,nq9", "f32,nq200", "sq8,nq9", "pq,nq9"):
        f[f"search_flat_probed[{t}]"] = "probed"
    for t in ("search_sq8[nom,nq4]", "search_sq8[nom,nq6]", "search_sq8[nom,nq6]@2", "search_rabitq[nq4]", "search_pq_adc[nom,nq8]"):
        f[t] = "scans"
    for dim in (32, 768):
        for e in ("search_hnsw", "search_hnsw@2", "search_hnsw_stats", "search_hnsw_pq", "search_hnsw_filtered", "search_hnsw_predicate",
                  "search_hnsw_brute[0]", "search_hnsw_brute[1]", "search_vamana[0]", "search_vamana[0]@2", "search_vamana[1]",
                  "search_vamana[2]", "search_vamana[3]", "search_vamana_stats", "search_vamana_filtered", "search_vamana_threshold",
                  "search_hnsw_pq_stats", "search_hnsw_filtered_stats", "search_hnsw_predicate_stats", "search_vamana_stats[1]",
                  "search_vamana_stats[2]", "search_vamana_stats[3]", "search_vamana_filtered_stats", "search_vamana_threshold_stats",
                  "rerank", "score_candidates"):
            base, _, tag = e.partition("@")
            f[f"{base}[{dim}]" + ("@" + tag if tag else "")] = "walks"
    return f


FAMILY_OF = _names()
ALL = sorted(n for n in FAMILY_OF if "@" not in n)
DEVICE_ONLY = [n for n in ALL if "_stats" not in n]   # every buffer device-resident (per-query stats are a host array)
TWO_STREAMS = ["sq8_encode[128]", "pq_asym[768,96,256]", "search_flat[128,nq200]", "search_sq8[nom,nq6]", "search_hnsw[32]",
               "search_vamana[0][32]"]
MIXED = ["sq8_encode[128]", "pq_decode[768,96,256]", "search_flat[128,nq8]", "binary_hamming[128]"]

# With every buffer device-resident an entry only enqueues (include/vecgo_hip.h, "Enqueue-only entry points"): the call returns
# while the producer of its inputs is still running.  These cases wait on the stream inside the call instead — the brute
# search reads its filter's population count and its redo flags back, a nominated batch reads the proofs' flags back.
WAITING = frozenset(["search_hnsw_brute[0][32]", "search_hnsw_brute[0][768]", "search_hnsw_brute[1][32]", "search_hnsw_brute[1][768]",
                     "search_pq_adc[nom,nq8]", "search_sq8[nom,nq6]"])
ENQUEUE_ONLY = frozenset(DEVICE_ONLY) - WAITING


# How many of a case's skewed caller buffers the library passes through a scratch block (vg::kStage16): all of them, except at
# the call sites that test the pointer and keep it for an element-wise kernel (vg::kAnyAlign; DESIGN.md has the table).
# By entry; 0 = the entry stages nothing and its fallback kernels read and write the skewed buffers themselves.
STAGED = {"sq8_encode": 0, "sq8_decode": 0, "sq8_l2": 2, "int4_encode": 0, "int4_decode": 0, "int4_l2_distance": 2,
          "int4_l2_distance_batch": 2, "pq_encode": 1, "pq_decode": 0, "pq_asym": 2, "pq_adc_lookup": 0, "opq_decode": 1, "opq_asym": 2,
          "rabitq_distance": 2}


def staged_buffers(ctx):
    """misaligned device buffers staged since the last read (vg_profile_read's counter)"""
    return ctx.profile_read("staged_device_buffers")[0]


@pytest.fixture(scope="module")
def world(vg, ctx):
    return World(vg, ctx)


def check(got, want, what):
    from tests.devbuf import raw, to_host
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, Ragged):
            a = to_host(g)
            for qi, row in enumerate(w.rows):
                r = row.size
                assert np.array_equal(a[qi, :r].view(np.uint32), np.asarray(row).view(np.uint32)), (what, i, qi, a[qi], row)
                if w.pad_invalid:
                    assert np.all(a[qi, r:].view(np.uint32) == INVALID), (what, i, qi)
        else:
            a, b = raw(g), raw(w)
            assert a.size == b.size and np.array_equal(a, b), (what, i, int((a != b).sum()) if a.size == b.size else (a.size, b.size))


def buffers(db, case, ins_how, outs_how):
    make = {"whole": db.whole, "skew": lambda a: db.offset_like(a, db.skew_bytes_of(a)), "host": lambda a: np.array(a, copy=True)}
    b = {k: make[ins_how](v) for k, v in case.ins.items()}
    out = tuple(make[outs_how](np.zeros(shape, dt)) for shape, dt in case.outs) if case.outs else None
    return b, out


# ---- Part A -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_odd_offsets_give_the_oracles_bits(torch, db, ctx, world, name):
    case = world[name]
    b, out = buffers(db, case, "whole", "whole")
    staged_buffers(ctx)
    aligned = case.call(b, out, None)
    torch.cuda.synchronize()
    assert staged_buffers(ctx) == 0, (name, "an aligned caller's buffers are used where they lie")
    check(aligned, case.want, (name, "aligned"))
    b, out = buffers(db, case, "skew", "skew")
    for t in list(b.values()) + list(out or ()):
        assert t.data_ptr() % 16 != 0
    ctx.profile_enable(True)
    try:
        skewed = case.call(b, out, None)
        torch.cuda.synchronize()
        launched = {sc: ctx.profile_read(sc)[0] for sc in SCOPES}
    finally:
        ctx.profile_enable(False)
    staged, expect = staged_buffers(ctx), STAGED.get(name.split("[")[0], len(case.ins) + len(case.outs))
    assert (staged == 0) if expect == 0 else (staged >= expect), (name, "staged", staged, "expected", expect)
    check(skewed, case.want, (name, "skewed"))
    check(skewed, aligned, (name, "skewed vs aligned"))
    for sc in case.prof:
        assert launched[sc] >= 1, (name, sc, launched)


def test_setters_copy_from_skewed_device_tensors(torch, db, vg, ctx, world):
    """set_vectors, set_pq_codes, set_sq8_codes and set_int4_codes copy into storage the index owns: from views at odd
    offsets, then one search over each."""
    n, dim = N_GRAPH, 128
    rng = np.random.default_rng(12000)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((4, dim)).astype(np.float32)
    skew = lambda a: db.offset_like(a, db.skew_bytes_of(a))
    idx = vg.Index(ctx, n, dim)
    idx.set_vectors(skew(base))
    opq, pq = world._random_pq(rng, dim, 16, 256)
    pcodes = opq.encode_batch(base)
    idx.set_pq_codes(pq, skew(pcodes))
    osq = o.ScalarQuantizer(dim); osq.train(base)
    sq = vg.ScalarQuantizer(ctx, dim); sq.train(base)
    scodes = osq.encode_batch(base)
    idx.set_sq8_codes(sq, skew(scodes))
    oiq = o.Int4Quantizer(dim); oiq.train(base)
    iq = vg.Int4Quantizer(ctx, dim); iq.train(base)
    icodes = oiq.encode_batch(base)
    idx.set_int4_codes(iq, skew(icodes))
    g, entry = graphs.build_vamana(base, r=16, seed=1)
    idx.set_vamana_graph(g, entry)
    ov = o.VamanaIndex(g, entry, dim, o.VAMANA_INT4, codes=icodes, int4_table=oiq.table)
    got = {"flat": idx.search_flat(q, K), "pq": idx.search_pq_adc(q, K), "sq8": idx.search_sq8(q, K), "int4": idx.search_vamana(q, K, kind=3)}
    for i in range(4):
        want = {"flat": o.flat_search_f32(base, dim, q[i], K), "pq": o.flat_search_pq(opq, pcodes, q[i], K),
                "sq8": o.flat_search_sq8(osq, scodes, q[i], K), "int4": ov.search(q[i], K)[:2]}
        for key, (eid, esc) in want.items():
            ids, sc = got[key]
            assert np.array_equal(ids[i, :eid.size], eid), (key, i)
            assert np.array_equal(sc[i, :eid.size].view(np.uint32), esc.view(np.uint32)), (key, i)


# ---- Part B -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def side(torch, db):
    """a fresh non-blocking stream, with the delay chain warmed up on it (the first product loads the BLAS kernels)"""
    s = torch.cuda.Stream()
    db.enqueue_delay(s, 2)
    s.synchronize()
    return s


@pytest.mark.parametrize("name", DEVICE_ONLY)
def test_callers_stream_orders_the_call(torch, db, world, side, name):
    case = world[name]
    staging = {k: db.whole(v) for k, v in case.ins.items()}
    b, out = buffers(db, case, "whole", "whole")
    keys = list(b)
    torch.cuda.synchronize()    # setup used the default stream; from here on only `side`
    s = side
    with torch.cuda.stream(s):
        warm = case.call(b, out, s)    # first use of this stream by this entry: its scratch blocks and arena exist afterwards
        warm = tuple(w.clone() for w in warm)
        for t in out or ():
            db.poison_(t)
    ev = db.late_inputs(s, [b[k] for k in keys], [staging[k] for k in keys], [case.poison.get(k) for k in keys])
    assert not ev.query(), f"{name}: the ordering was not exercised — the producer of the inputs had finished before the call"
    with torch.cuda.stream(s):
        res = case.call(b, out, s)
        waited = ev.query()
        kept = tuple(r.clone() for r in res)
        for t in list(b.values()) + [r for r in res if r is not b.get(case.inout)]:
            db.poison_(t)
    s.synchronize()
    check(warm, case.want, (name, "side stream"))
    check(kept, case.want, (name, "late inputs"))
    if name in ENQUEUE_ONLY:
        assert not waited, f"{name}: documented as enqueue-only, but the call returned after the producer of its inputs had finished"
    else:
        assert waited, f"{name}: documented as waiting for the stream, but the call returned before its inputs existed"


@pytest.mark.parametrize("mode", ["back_to_back", "threads"])
@pytest.mark.parametrize("name", TWO_STREAMS)
def test_two_streams_share_no_scratch(torch, db, world, name, mode):
    """The same entry on two side streams with different inputs, no host wait in between; both streams are held back by one
    event behind a delay on a third, so their work starts together and overlaps.  Every caller buffer is a skewed view: where
    the library stages those, each call holds scratch blocks keyed by its own stream.  What each entry can show: sq8_encode
    keeps skewed pointers for its element kernel and takes no scratch at all, so it checks only that two streams' launches do
    not disturb each other; pq_asym stages its query and output; the searches add their own temporaries and arenas.
    search_sq8[nom,nq6] waits for its stream inside the call, so back to back its second call is issued after the first has
    drained and only the two threads overlap."""
    cases = (world[name], world[name + "@2"])
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    gate = torch.cuda.Stream()
    bufs = [buffers(db, c, "skew", "skew") for c in cases]
    torch.cuda.synchronize()
    for c, (b, out), s in zip(cases, bufs, streams):    # first use of each stream
        with torch.cuda.stream(s):
            c.call(b, out, s)
    for s in streams:
        s.synchronize()
    db.enqueue_delay(gate, 2)
    gate.synchronize()
    db.enqueue_delay(gate)
    ev = torch.cuda.Event()
    ev.record(gate)
    for s in streams:
        s.wait_event(ev)
    assert not ev.query(), f"{name}: the two streams were not held back — nothing overlaps"
    results = [None, None]

    def run(i):
        with torch.cuda.stream(streams[i]):
            results[i] = cases[i].call(bufs[i][0], bufs[i][1], streams[i])
    if mode == "back_to_back":
        run(0); run(1)
    else:
        threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    for s in streams:
        s.synchronize()
    for i in range(2):
        assert results[i] is not None, (name, mode, i)
        check(results[i], cases[i].want, (name, mode, "stream", i))


# ---- Part C -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ins_how,outs_how", [("host", "whole"), ("whole", "host")])
@pytest.mark.parametrize("name", MIXED)
def test_mixed_host_and_device_buffers(torch, db, world, name, ins_how, outs_how):
    case = world[name]
    s = torch.cuda.Stream()
    b, out = buffers(db, case, ins_how, outs_how)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        res = case.call(b, out, s)
    s.synchronize()    # device-resident outputs: the call itself does not wait for them
    check(res, case.want, (name, ins_how, outs_how))


@pytest.mark.parametrize("queries", ["whole", "host"])
def test_mixed_walk_with_stats(torch, db, world, queries):
    """search_hnsw with stats has no out=: device queries give device ids / scores beside the host stats array; host queries
    give host results."""
    case = world["search_hnsw_stats[32]"]
    s = torch.cuda.Stream()
    b, _ = buffers(db, case, queries, "whole")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        res = case.call(b, None, s)
    s.synchronize()
    assert isinstance(res[0], torch.Tensor) == (queries == "whole") and isinstance(res[2], np.ndarray)
    check(res, case.want, ("search_hnsw_stats[32]", queries))
