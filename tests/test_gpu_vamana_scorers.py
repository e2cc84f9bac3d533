"""Every node scorer of the Vamana walk (vg_node_score.hpp) under every result-set form of vamana_search_kernel, against the oracle's
walk over the same graph: ids, score bits, padding and the (nodes_visited, distance_computations, pops) counters.

The shapes are the ones at which a scorer takes another path:
  fp32        dim 20 (one partial 16-lane pass) and 100; L2 and Dot
  PQ table    sub-dimension 4, m = 8 (scalar loop), 16 (one 16-group), 48 (the 32- and 16-chunks), 96 (the 96-chunk)
  PQ direct   sub-dimension 8, m = 3 (pair + odd scalar tail), 5, 16 (one 16-group), 48 (32-chunk + 16-chunk)
  RaBitQ      dim 40 (2 words: tail loop only), 512 (16 words: unrolled part only), 576 (18 words: both)
  INT4        dim 47 and 100 from the table, dim 32 and 96 evaluated in place
k = 10 / 100 / 600: the register list, the sorted LDS list, the 64-ary heap with its sort; each unfiltered and with a 30 % filter
per query.  The STRICT pass (the reference's CandidateHeap, vg_cand_replay.hpp) of the instances no other test reaches — the PQ
table form, both INT4 forms — runs on a query with an Inf in one coordinate."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import graphs
from tests.test_gpu_vamana_large_k import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


N, R, NQ = 700, 12, 6
KS = (10, 100, 600)

F32 = [("f32", 20, 0), ("f32", 100, 0), ("f32", 20, 2)]
PQ_TABLE = [("pq", 32, 8), ("pq", 64, 16), ("pq", 192, 48), ("pq", 384, 96)]
PQ_DIRECT = [("pq", 24, 3), ("pq", 40, 5), ("pq", 128, 16), ("pq", 384, 48)]
RABITQ = [("rabitq", 40, 0), ("rabitq", 512, 0), ("rabitq", 576, 0)]
INT4_TABLE = [("int4", 47, 0), ("int4", 100, 0)]
INT4_DIRECT = [("int4", 32, 0), ("int4", 96, 0)]
KIND = {"f32": 0, "pq": 1, "rabitq": 2, "int4": 3}

_cases = {}


def case(vg, ctx, scorer, dim, arg):
    """(GPU index, oracle walk, queries, per-query masks) of one scorer shape, built once and left unchanged.
    arg: the metric (fp32) or m (PQ)"""
    key = (scorer, dim, arg)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(1000 * dim + 10 * arg + KIND[scorer])
    base = rng.standard_normal((N, dim)).astype(np.float32)
    # (the graph's construction is not under test: near neighbours by the first 32 coordinates keep the set-up short)
    g, entry = graphs.build_vamana(base[:, :32], r=R, seed=dim)
    metric = arg if scorer == "f32" else 0
    idx = vg.Index(ctx, N, dim, vg.Metric(metric))
    idx.set_vamana_graph(g, entry)
    if scorer == "f32":
        idx.set_vectors(base)
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_F32, metric=metric, base=base)
    elif scorer == "pq":
        m, sub = arg, dim // arg
        opq = o.ProductQuantizer(dim, m, 256)
        opq.set_codebooks(rng.integers(-128, 128, m * 256 * sub).astype(np.int8), (rng.random(m) * 0.02 + 0.005).astype(np.float32),
                          ((rng.random(m) * 2 - 1) * 0.1).astype(np.float32))
        codes = opq.encode_batch(base)
        pq = vg.ProductQuantizer(ctx, dim, m, 256)
        pq.set_codebooks(opq.codebooks, opq.scales, opq.offsets)
        idx.set_pq_codes(pq, codes)
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_PQ, pq=opq, codes=codes)
    elif scorer == "rabitq":
        codes = o.rabitq_encode_batch(base, dim)
        idx.set_rabitq_codes(codes)
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_RABITQ, codes=codes)
    else:
        ref = o.Int4Quantizer(dim)
        ref.train(base)
        codes = ref.encode_batch(base)
        iq = vg.Int4Quantizer(ctx, dim)
        iq.train(base)
        idx.set_int4_codes(iq, codes)
        ov = o.VamanaIndex(g, entry, dim, o.VAMANA_INT4, codes=codes, int4_table=ref.table)
    q = rng.standard_normal((NQ, dim)).astype(np.float32)
    masks = rng.random((NQ, N)) < 0.3
    _cases[key] = (idx, ov, q, masks, metric)
    return _cases[key]


@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask30"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("scorer,dim,arg", F32 + PQ_TABLE + PQ_DIRECT + RABITQ + INT4_TABLE + INT4_DIRECT)
def test_scorer_under_every_result_set(vg, ctx, scorer, dim, arg, k, masked):
    idx, ov, q, masks, metric = case(vg, ctx, scorer, dim, arg)
    check(idx, ov, q, k, KIND[scorer], mask=masks if masked else None, metric=metric)


@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask30"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("scorer,dim,arg", PQ_TABLE + INT4_TABLE + INT4_DIRECT)
def test_strict_pass_of_table_and_int4_scorers(vg, ctx, scorer, dim, arg, k, masked):
    """one query in six with an Inf in one coordinate: its distances are Inf or NaN, so the second pass answers it with the
    reference's CandidateHeap (float comparisons, neighbour by neighbour); the other five return from that pass at once"""
    idx, ov, q, masks, metric = case(vg, ctx, scorer, dim, arg)
    q = q.copy()
    q[2, dim // 3] = np.inf
    est = ov.search(q[2], k)[2]
    assert est.pops >= 1                                     # the oracle answers this input
    check(idx, ov, q, k, KIND[scorer], mask=masks if masked else None, metric=metric)
