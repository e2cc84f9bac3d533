"""ProductQuantizer Train at the seams of its k-means++ seeding (k_pq_train.hip: pq_kmeanspp_kernel), reached on purpose
(tests/pq_train_cases.py builds the inputs, tests/test_pq_train_cases_cpu.py shows they are what they claim):
  A  block prefixes in global memory (n > 262 144): the chunked scan with its carried running sum, the pick and the
     in-block walk reading pref[], the scratch of a second sub-quantizer slot, a sub-quantizer range;
  B  the software-pipelined distance pass of sub-vector dims 4 / 8 / 16 at one trip, one block past it, a ragged first
     block of wave 1, a third load and four trips, the generic pass around one and two blocks per wave, and the row tail
     of pq_assign_vec_kernel;
  C  the walk's fallback: the picked block's sequential sum ends below the target;
  D  all rows identical (pq_quantize_kernel's equal extremes), k = 1 and 2, fewer distinct sub-vectors than k, iters = 0.
Every expected value is the oracle's, every comparison exact; nothing is compared with another GPU path."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import pq_train_cases as pc

pytestmark = pytest.mark.gpu


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def vg():
    import vecgo_amd
    return vecgo_amd


@pytest.fixture(scope="module")
def ctx(vg):
    return vg.Context(0)


_WANT = {}


def oracle_train(case, iters):
    """The oracle's (codebooks, scales, offsets), read-only; kept for the one result two tests share (A2's sd = 8 rows)."""
    keep = case.name in ("A2-sd8", "A4-subset")
    key = ("A2-sd8", iters)
    if keep and key in _WANT:
        return _WANT[key]
    opq = o.ProductQuantizer(case.dim, case.m, case.k)
    opq.train(case.rows(), iters=iters, seed=case.seed)
    want = (opq.codebooks, opq.scales, opq.offsets)
    for a in want:
        a.setflags(write=False)
    if keep:
        _WANT[key] = want
    return want


def assert_same(case, iters, got, want, subs):
    """got / want: (codebooks, scales, offsets) of the sub-quantizers `subs`."""
    (cb, sc, of), (wcb, wsc, wof) = got, want
    per = case.k * case.sd
    what = (case.name, f"iters={iters}")
    assert cb.shape == wcb.shape and cb.dtype == np.int8
    bad = np.flatnonzero(cb != wcb)
    assert bad.size == 0, (*what, f"{bad.size} codebook bytes differ, sub-quantizers "
                           f"{sorted({subs[i] for i in (bad // per).tolist()})}")
    assert np.array_equal(bits(sc), bits(wsc)), (*what, "scales", [subs[i] for i in np.flatnonzero(bits(sc) != bits(wsc))])
    assert np.array_equal(bits(of), bits(wof)), (*what, "offsets", [subs[i] for i in np.flatnonzero(bits(of) != bits(wof))])


CASES = [(case, iters) for case in pc.all_cases() for iters in case.iters]


@pytest.mark.parametrize("case,iters", CASES, ids=[f"{case.name}-it{iters}" for case, iters in CASES])
def test_train_matches_the_oracle(vg, ctx, case, iters):
    x = case.rows()
    assert x.shape == (case.n, case.dim)
    want = oracle_train(case, iters)
    pq = vg.ProductQuantizer(ctx, case.dim, case.m, case.k)
    pq.train(x, iters=iters, seed=case.seed)
    assert pq.is_trained()
    assert_same(case, iters, pq.codebooks(), want, list(range(case.m)))


def test_sub_quantizer_range_with_prefixes_in_global_memory(vg, ctx):
    """A4: train_subset(x, 1, 1) on A2's sd = 8 rows — the global sub-quantizer 1 (its RNG stream, its columns) in
    scratch slot 0."""
    case = pc.a4_case()
    (iters,) = case.iters
    wcb, wsc, wof = oracle_train(case, iters)
    per = case.k * case.sd
    pq = vg.ProductQuantizer(ctx, case.dim, case.m, case.k)
    pq.train_subset(case.rows(), 1, 1, iters=iters, seed=case.seed)
    assert not pq.is_trained()
    assert_same(case, iters, pq.codebooks_range(1, 1), (wcb[per:2 * per], wsc[1:2], wof[1:2]), [1])
