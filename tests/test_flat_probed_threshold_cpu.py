"""No-GPU checks of vg_search_flat_probed_threshold / vg_segment_search_threshold (Engine.SearchThreshold over flat segments
with codes and IVF partitions): the reference composition the GPU tests compare with (tests/probed_threshold_ref.py) against
hand-made cases, and the two symbols through every layer — header, the minor-13 note, the built library, the bindings."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as o
from tests.probed_threshold_ref import L2, DOT, candidates, expected, rank_threshold
from vecgo_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("vg_search_flat_probed_threshold", "vg_segment_search_threshold")
INVALID = 0xFFFFFFFF


def two_partition_case():
    """internal/engine/batch_test.go:47-67 — rows {1,0}, {0,1}, {1,1}, query {1,0}, L2 — laid into two partitions as the flat
    writer would: partition 0 holds {1,0} and {1,1} (rows 0, 1), partition 1 holds {0,1} (row 2)"""
    base = np.array([[1, 0], [1, 1], [0, 1]], np.float32)
    cent = np.array([[1, 0.5], [0, 1]], np.float32)
    off = np.array([0, 2, 3], np.uint32)
    return o.FlatSegment(base, 2, centroids=cent, part_offsets=off), np.array([1, 0], np.float32)


def test_reference_case_in_two_partitions():
    seg, q = two_partition_case()
    # one probe: partition 0 only (its centroid is the closer one)
    ids, sc, kept = expected(seg, q, 0.5, 10, nprobes=1)
    assert kept == 1 and ids[:1].tolist() == [0] and sc[:1].tolist() == [0.0]
    ids, sc, kept = expected(seg, q, 1.1, 10, nprobes=1)
    assert kept == 2 and ids[:2].tolist() == [0, 1] and sc[:2].tolist() == [0.0, 1.0]
    ids, sc, kept = expected(seg, q, 2.0, 10, nprobes=1)   # {0,1} is within 2.0 but not probed
    assert kept == 2
    assert np.all(ids[2:] == INVALID) and np.all(np.isposinf(sc[2:]))
    # both probes: the boundary is kept
    ids, sc, kept = expected(seg, q, 2.0, 10, nprobes=2)
    assert kept == 3 and ids[:3].tolist() == [0, 1, 2] and sc[:3].tolist() == [0.0, 1.0, 2.0]
    # max_results cuts before the threshold does
    ids, sc, kept = expected(seg, q, 2.0, 2, nprobes=2)
    assert kept == 2 and ids.tolist() == [0, 1]
    # a NaN threshold keeps nothing
    assert expected(seg, q, np.nan, 10, nprobes=2)[2] == 0


@pytest.mark.parametrize("metric", [L2, DOT])
def test_without_rerank_an_infinite_threshold_is_the_search(metric):
    rng = np.random.default_rng(3)
    base = rng.standard_normal((200, 8)).astype(np.float32)
    cent = base[:3].copy()
    a = np.asarray(o.assign_partition_batch(base, cent, metric), np.int64)
    order = np.argsort(a, kind="stable")
    base = np.ascontiguousarray(base[order])
    off = np.searchsorted(a[order], np.arange(4)).astype(np.uint32)
    seg = o.FlatSegment(base, 8, metric=metric, centroids=cent, part_offsets=off)
    q = rng.standard_normal(8).astype(np.float32)
    t = rank_threshold(seg, q, "all", 20)
    assert np.isinf(t)
    for nprobes in (1, 2, 3):
        sid, ssc = seg.search(q, 20, nprobes)
        ids, sc, kept = expected(seg, q, t, 20, nprobes=nprobes, rerank=False)
        assert kept == sid.size and np.array_equal(ids[:kept], sid) and np.array_equal(sc[:kept].view(np.uint32), ssc.view(np.uint32))
        assert expected(seg, q, rank_threshold(seg, q, "none", 20), 20, nprobes=nprobes)[2] == 0
        # a threshold at rank r keeps at least r rows (equal scores stay together)
        t5 = rank_threshold(seg, q, 5, 20, nprobes=nprobes)
        assert expected(seg, q, t5, 20, nprobes=nprobes)[2] >= 5


def test_rerank_orders_by_exact_score():
    """SQ8 candidates re-scored: the scores are the fp32 rows' and ascending, the ids a permutation of the candidates"""
    rng = np.random.default_rng(4)
    base = rng.standard_normal((300, 12)).astype(np.float32)
    sq = o.ScalarQuantizer(12)
    sq.train(base)
    seg = o.FlatSegment(base, 12, sq=sq, codes=sq.encode_batch(base))
    q = rng.standard_normal(12).astype(np.float32)
    cid, _ = candidates(seg, q, 40)
    rid, rsc = candidates(seg, q, 40, rerank=True)
    assert sorted(cid.tolist()) == sorted(rid.tolist())
    assert np.all(np.diff(rsc) >= 0)
    assert np.array_equal(rsc.view(np.uint32), np.array([o.l2(q, base[i]) for i in rid], np.float32).view(np.uint32))


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_header_declares_it(symbol):
    assert symbol in _lib.declared_symbols()


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_minor_13_note_names_it(symbol):
    text = _lib.HEADER_PATH.read_text()
    note = re.search(r"Added at minor 13 without a bump(.*?)#define VG_ABI_MINOR (\d+)", text, flags=re.S)
    assert note and note.group(2) == "13"
    assert re.search(rf"\b{symbol}\b", note.group(1)), f"{symbol} is not in the minor-13 note"


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_library_exports_it(symbol):
    assert hasattr(_lib.load(), symbol)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_bindings_call_it(symbol):
    assert f"_lib.{symbol}(" in (ROOT / "vecgo_amd" / "api.py").read_text()
    assert f"C.{symbol}(" in (ROOT / "go" / "segment" / "resident.go").read_text()


def test_cpp_mirror_has_the_probed_threshold_search():
    text = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert "SearchProbedThreshold" in text and "vg_search_flat_probed_threshold(" in text


def test_null_handles_are_argument_errors():
    import ctypes as C
    lib = _lib.load()
    z = C.c_void_p(0)
    assert lib.vg_search_flat_probed_threshold(None, z, C.c_int64(1), z, C.c_int32(4), C.c_int32(1), C.c_int32(0), C.c_int32(0), None,
                                               C.c_int64(0), z, z, z, None) == -1
    assert lib.vg_segment_search_threshold(None, z, C.c_int64(1), z, C.c_int32(4), C.c_int32(1), C.c_int32(0), None, C.c_int64(0), z, z,
                                           z, None) == -1
