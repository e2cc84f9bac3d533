"""tests/probe_cases.py against the constants and dispatch expressions it restates (vg_flat_gemm.hpp, vg_internal.hpp, k_probe.hip,
k_flat.hip: a retune of a tile, a cap or a gate fails here, so the cases get revisited), every builder's own conditions — exact
pair counts per partition under the ORACLE's probe selection, more than GEMM_CAP rows under the sampled threshold — and the
oracle's answer to every query the GPU test compares with it."""
import pathlib
import re

import numpy as np
import pytest

from oracle import oracle as o
from tests import probe_cases as pc

CSRC = pathlib.Path(__file__).resolve().parents[1] / "vecgo_amd" / "csrc"


def src(name):
    return (CSRC / name).read_text()


def constant(text, pattern):
    found = re.findall(pattern, text, flags=re.M)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_constants_are_the_sources():
    gemm, internal, probe, flat = src("vg_flat_gemm.hpp"), src("vg_internal.hpp"), src("k_probe.hip"), src("k_flat.hip")
    bm, bn = re.search(r"^constexpr int kGemmBM = (\d+), kGemmBN = (\d+),", gemm, flags=re.M).groups()
    assert (int(bm), int(bn)) == (pc.GEMM_BM, pc.GEMM_BN)
    g32 = constant(gemm, r"^constexpr int kG32BM = (\d+);")
    rb = constant(gemm, r"^#define VG_PROBE_RB (\d+)$")
    assert len(re.findall(r"^constexpr int kProbeRB = VG_PROBE_RB;", gemm, flags=re.M)) == 1
    assert "VG_PROBE_RB" not in src("Makefile")                 # nothing in the build overrides the macro
    assert rb * g32 == pc.SMALL_TILE_Q
    assert constant(internal, r"^constexpr int kProbeQB = (\d+);") == pc.PROBE_QB
    assert constant(internal, r"^constexpr int kProbeGemmMaxK = (\d+);") == pc.GEMM_MAX_K
    assert constant(probe, r"^constexpr int kProbeSampleStride = (\d+);") == pc.SAMPLE_STRIDE
    assert constant(probe, r"^constexpr int64_t kProbeSmallMax = (\d+);") == pc.SMALL_MAX
    assert constant(flat, r"^constexpr int kProbeGemmCap = (\d+);") == pc.GEMM_CAP
    # the thresholds hidden_from_sample argues with: the 8th best sampled score up to k = 48, a deeper (higher) one above
    assert constant(flat, r"^constexpr int kGemmMaxK = (\d+);") == 48
    assert "int probe_gemm_sel_k(int k, bool bf16) { return k <= kGemmMaxK ? 8 : std::min(64, std::max(8, ((bf16 ? 5 : 3) * k + 7) / 8)); }" in flat


def test_dispatch_is_the_source():
    probe = src("k_probe.hip")
    shape = re.search(r"const bool gemm_shape = (.*?);", probe, flags=re.S).group(1)
    assert f"pairs <= {pc.MAX_PAIRS}" in shape and "k <= vg::kProbeGemmMaxK" in shape
    assert re.search(rf"pairs >= {pc.MIN_PAIRS_PER_PART} \* static_cast<int64_t>\(parts\)", shape)
    assert "!vg::hook(vg::kHookProbeNoGroup) && !vg::hook(vg::kHookProbeNoGemm)" in shape
    assert len(re.findall(r"small = cnt <= kProbeSmallMax;", probe)) == 1
    group_ok = re.search(r"const bool group_ok = (.*?);", probe).group(1)
    assert group_ok == f"(c.whole ? nq >= 4 : pairs >= {pc.GROUP_MIN_PAIRS}) && !vg::hook(vg::kHookProbeNoGroup)"
    # the small tiles hold kProbeRB * kG32BM queries, the grids' skew terms divide by the tiles' query counts
    assert "const int64_t mt64 = (cnt + kProbeRB * kG32BM - 1) / (kProbeRB * kG32BM);" in probe
    assert "grids[0] = sum_s + (pairs / vg::kGemmBM) * max_s;" in probe and "grids[1] = sum_m + (pairs / vg::kGemmBM) * max_m;" in probe
    assert "grids[2] += (pairs / (vg::kProbeRB * vg::kG32BM)) * max_nst;" in probe
    assert "grids[3] += (pairs / (vg::kProbeRB * vg::kG32BM)) * max_nt;" in probe
    # the grouped scan's grid bound and the bucketing kernels' partitions per thread
    assert "std::min<int64_t>(cpairs, cpairs / vg::kProbeQB + parts)" in probe
    assert len(re.findall(rf"const int per = \(parts \+ {pc.BUCKET_THREADS - 1}\) / {pc.BUCKET_THREADS};", probe)) == 2
    # an overflowing pair is answered by the exact kernel through qfail (k <= 64) or the subset search (k > 64)
    assert "return vg::launch_topk_merge(partial, nq, c.lists, k, c.dot, c.oid, c.osc, st, qfail);" in probe
    assert "if (sq8 || k > 64) {" in probe
    assert pc.takes_gemm(12 * 7, 7) and not pc.takes_gemm(12 * 7 - 1, 7) and not pc.takes_gemm(65536, 7)
    assert not pc.takes_gemm(1000, 7, k=161) and pc.takes_group(16) and not pc.takes_group(15)


def test_block_model_by_hand():
    # one partition of 1500 rows (12 row tiles, 2 sampled): 512 pairs = 4 small query tiles, 513 = 5 tiles of 128 x 128 with the
    # row tiles rounded up to 8 and 16
    assert pc.gemm_blocks([512], [1500])[0] == (0, 0, 4 * 2, 4 * 12)
    assert pc.gemm_blocks([513], [1500])[0] == (5 * 8, 5 * 16, 0, 0)
    assert pc.gemm_blocks([7, 0, 9], [0, 500, 129])[0] == (0, 0, 1, 2)
    for rows, nt, nst in ((1, 1, 1), (128, 1, 1), (129, 2, 1), (1024, 8, 1), (1025, 9, 2)):
        assert pc.gemm_blocks([1], [rows])[0] == (0, 0, nst, nt)
    assert pc.scan_groups([1] * 29 + [61]) == (37, 41) and pc.scan_groups([8, 9, 0, 16]) == (5, 8)


def check_case(case, ks=(10,)):
    """the case as the GPU test uses it: a legal segment, the pair counts of the oracle's own probe selection, and an oracle
    answer for every named query"""
    parts, dim = case.cent.shape
    assert case.off.dtype == np.uint32 and case.off.size == parts + 1 and case.off[-1] == case.x.shape[0] <= 40000
    assert np.all(np.diff(case.off.astype(np.int64)) >= 0) and dim in (32, 64)
    pr = pc.probes_of(case.q, case.cent, case.nprobes, case.metric)
    assert np.array_equal(np.bincount(pr.ravel(), minlength=parts), case.pair_counts)
    assert case.gemm == pc.takes_gemm(pr.size, parts, max(ks))
    assert len(case.named) <= 14 and 0 in case.named and case.q.shape[0] - 1 in case.named
    seg = o.FlatSegment(case.x, dim, metric=case.metric, centroids=case.cent, part_offsets=case.off)
    rows = np.diff(case.off.astype(np.int64))
    for i in case.named:
        for k in ks:
            ids, sc = seg.search(case.q[i], k, case.nprobes)
            assert ids.size == min(k, int(rows[pr[i]].sum()))
            key = -sc if case.metric != 0 else sc
            assert np.all(np.diff(key) >= 0)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("nprobes", [1, 2])
def test_tile_kind_case(metric, nprobes):
    case = pc.tile_kind_case(metric, nprobes)
    check_case(case)
    want = [511, 512, 513, 129, 128, 1] if nprobes == 1 else [511, 512, 1794, 129, 128, 514]
    assert case.pair_counts.tolist() == want and case.gemm


@pytest.mark.parametrize("nprobes", [1, 2])
def test_skew_case(nprobes):
    case = pc.skew_case(nprobes)
    check_case(case)
    assert sorted(case.pair_counts.tolist())[-2:] == ([0, 1300] if nprobes == 1 else [1300, 1300]) and case.gemm
    assert -(-1300 // pc.GEMM_BM) == 11 and case.pair_counts[np.argmax(np.diff(case.off.astype(np.int64)))] == 1300


@pytest.mark.parametrize("metric", [0, 2])
def test_row_seam_case(metric):
    case, target = pc.row_seam_case(metric)
    check_case(case, ks=(10, 100, 128))
    assert np.diff(case.off.astype(np.int64)).tolist() == [1, 127, 128, 129, 0, 1024, 1025, 1023, 0, 2]
    assert case.pair_counts.tolist() == pc.ROW_SEAM_COUNTS and case.gemm
    assert {int(target[i]) for i in case.named} == {p for p in range(10) if pc.ROW_SEAM_COUNTS[p]}


@pytest.mark.parametrize("parts,nq,nprobes,gemm", [(1500, 2400, 8, True), (1025, 20, 4, False)])
def test_many_parts_case(parts, nq, nprobes, gemm):
    case = pc.many_parts_case(parts, nq, nprobes)
    check_case(case)
    assert case.gemm == gemm and pc.takes_group(nq * nprobes)
    rows = np.diff(case.off.astype(np.int64))
    assert np.all(rows[6::7] == 0) and np.all(np.delete(rows, np.arange(6, parts, 7)) == 8)


@pytest.mark.parametrize("variant", ["ones", "ones2", "full"])
def test_group_bound_case(variant):
    case = pc.group_bound_case(variant)
    check_case(case)
    got = sorted(case.pair_counts.tolist())
    assert got == {"ones": [1] * 29 + [61], "ones2": [1] * 28 + [17, 45], "full": [8] * 15 + [9] * 15}[variant]
    assert not case.gemm


@pytest.mark.parametrize("duplicates", [False, True])
def test_overflow_case(duplicates):
    case, below = pc.overflow_case(duplicates)
    check_case(case, ks=(10, 100))
    assert below >= pc.GEMM_CAP + 200 and case.gemm and case.q.shape[0] == 200
    seg = o.FlatSegment(case.x, 32, centroids=case.cent, part_offsets=case.off)
    ids, sc = seg.search(case.q[pc.OVERFLOW_AT], 100, 1)
    tile = (ids.astype(np.int64) - int(case.off[1])) // pc.GEMM_BN
    assert np.all(tile % pc.SAMPLE_STRIDE != 0)                    # the answer lies in the tiles the sample skips
    if duplicates:
        assert np.unique(sc).size == 1 and np.all(np.diff(ids.astype(np.int64)) > 0)       # one long tie, resolved by row id
