"""The pre-filter search, the part that needs no GPU: tests/prefilter_ref.py (the engine's loop of search.go:602-736 for one
segment) pinned against the oracle's flat segment on finite data, one NaN case in which Pop-then-Push and ReplaceTop answer
differently, and the header's / bindings' new surface."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as o
from tests import prefilter_ref as ref

ROOT = Path(__file__).resolve().parents[1]
NEW = ("vg_mask_to_rows", "vg_search_flat_prefilter")


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("metric", [o.METRIC_L2, o.METRIC_COSINE, o.METRIC_DOT])
@pytest.mark.parametrize("dup", [1, 8])
def test_ref_equals_the_flat_segment_on_finite_data(metric, dup):
    """finite scores are totally ordered by (score, row id): the heap policy cannot matter, and the engine's loop over the
    listed rows answers what flat.Segment.Search answers under the same filter"""
    rng = np.random.default_rng(17 + metric + dup)
    n, dim = 400, 70
    x = rng.standard_normal((n // dup, dim)).astype(np.float32)
    x = np.repeat(x, dup, axis=0)[rng.permutation(n)] if dup > 1 else x   # duplicated rows: equal scores, ties by row id
    seg = o.FlatSegment(x, dim, metric=metric)
    for keep in (0.5, 0.03):
        m = rng.random(n) < keep
        hits = int(m.sum())
        for q in rng.standard_normal((3, dim)).astype(np.float32):
            for k in (1, max(hits - 1, 1), hits, hits + 5, 64):
                want_i, want_s = seg.search(q, k, 0, mask=m)
                for policy in ("pop_push", "replace_top"):
                    got_i, got_s = ref.search(x, dim, metric, q, k, m, policy)
                    assert np.array_equal(got_i, want_i), (metric, dup, keep, k, policy)
                    assert np.array_equal(bits(got_s), bits(want_s)), (metric, dup, keep, k, policy)
                assert got_i.size == min(k, hits)


def nan_case():
    """L2 scores 9, NaN, 4, 1, 2.25 in row order, k = 3.  The NaN enters while the heap fills and sits as the root's first
    child, where it stops every sift.  At 1: ReplaceTop leaves [1, NaN, 4] — the root is now the BEST item and 2.25 is turned
    away; Pop-then-Push leaves [4, NaN, 1] and 2.25 replaces the 4."""
    x = np.zeros((5, 4), np.float32)
    x[:, 0] = [3.0, np.nan, 2.0, 1.0, 1.5]
    return x, np.zeros(4, np.float32), 3


def test_pop_then_push_is_not_replace_top_once_a_score_is_nan():
    x, q, k = nan_case()
    m = np.ones(5, np.bool_)
    pi, ps = ref.search(x, 4, o.METRIC_L2, q, k, m, "pop_push")
    ri, rs = ref.search(x, 4, o.METRIC_L2, q, k, m, "replace_top")
    assert sorted(pi.tolist()) == [1, 3, 4] and sorted(ri.tolist()) == [1, 2, 3]
    assert set(pi.tolist()) != set(ri.tolist())
    # the same offers through the oracle's C heap (TryPushBounded = the ReplaceTop form) agree with the Python restatement
    h = o.CandidateHeap(False, cap=8)
    for r, s in enumerate(ref.scores_of(x, q, np.arange(5), o.METRIC_L2)):
        h.push(float(s), 0, r, k=k)
    popped = []
    while len(h):
        popped.append(h.pop()[2])
    h.close()
    assert popped[::-1] == ri.tolist()
    # a masked-out NaN row changes nothing: the row is never scored
    m[1] = False
    for policy in ("pop_push", "replace_top"):
        i, s = ref.search(x, 4, o.METRIC_L2, q, k, m, policy)
        assert i.tolist() == [3, 4, 2] and s.tolist() == [1.0, 2.25, 4.0]


def test_heap_restatement_follows_the_oracle_heap():
    """random offers with ties and NaNs, both directions: the Python heap and the oracle's C heap pop the same sequence"""
    rng = np.random.default_rng(5)
    for desc in (False, True):
        for k in (1, 4, 5, 21):
            s = rng.integers(0, 12, 200).astype(np.float32)
            s[rng.random(200) < 0.05] = np.nan
            h = o.CandidateHeap(desc, cap=64)
            for r, v in enumerate(s):
                h.push(float(v), 0, r, k=k)
            want = []
            while len(h):
                c = h.pop()
                want.append((c[2], c[0]))
            h.close()
            gi, gs = ref.offer_all(np.arange(200), s, k, desc, "replace_top")
            assert gi.tolist() == [w[0] for w in want][::-1], (desc, k)
            assert np.array_equal(bits(gs), bits([w[1] for w in want][::-1])), (desc, k)


def test_header_declares_exports_and_notes_the_new_entry_points():
    from vecgo_amd import _lib
    import vecgo_amd as vg
    text = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR 13\b", text)
    note = text[text.index("Added at minor 13 without a bump"):text.index("#define VG_ABI_MINOR")]
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.declared_symbols(), name
        assert hasattr(lib, name), f"libvecgo_hip.so does not export {name}"
        assert name in note, name
    assert "found by symbol lookup" in note[note.index("vg_mask_to_rows"):]
    assert int(re.search(r"#define VG_MASK_ROWS_TILE_ROWS (\d+)", text).group(1)) == vg.MASK_ROWS_TILE_ROWS
    assert int(re.search(r"#define VG_PREFILTER_CHUNK_ROWS (\d+)", text).group(1)) == vg.PREFILTER_CHUNK_ROWS
    for cite in ("search.go:500-737", "search.go:602-736", ":617-627", "search.go:725-733"):
        assert cite in text, cite
    enqueue = text[text.index("Enqueue-only entry points"):text.index("These WAIT for")]
    wait = text[text.index("These WAIT for"):text.index("Entry points in neither list")]
    assert "vg_mask_to_rows" in enqueue and "vg_search_flat_prefilter" not in enqueue
    assert "vg_search_flat_prefilter" in wait


def test_bindings_name_the_new_surface():
    import vecgo_amd as vg
    go = "".join(p.read_text() for p in sorted((ROOT / "go").rglob("*.go")))
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    api = (ROOT / "vecgo_amd" / "api.py").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, name
        assert f"{name}(" in hpp, name
        assert f"_lib.{name}" in api, name
    assert callable(vg.mask_to_rows) and "mask_to_rows" in vg.__all__
    assert callable(vg.Index.search_flat_prefilter)
    policy = (ROOT / "vecgo_amd" / "csrc" / "vg_cand_replay.hpp").read_text()
    assert "struct CandHeapPopPushPolicy" in policy


def test_malformed_calls_are_refused_without_a_device():
    """every refusal here comes before the library touches a device"""
    from vecgo_amd import _lib
    lib = _lib.load()
    assert lib.vg_search_flat_prefilter(None, None, C.c_int64(1), C.c_int32(1), None, C.c_int64(0), None, None, None) == -1
    assert b"NULL index" in lib.vg_last_error()
    assert lib.vg_mask_to_rows(None, None, C.c_int64(0), C.c_int64(1), C.c_int64(8), None, C.c_int64(0), None, None) == -1
    assert b"NULL context" in lib.vg_last_error()
    fake_ctx = C.c_void_p(0x10)   # never dereferenced below
    assert lib.vg_mask_to_rows(fake_ctx, None, C.c_int64(0), C.c_int64(-1), C.c_int64(8), None, C.c_int64(0), None, None) == -1
    assert lib.vg_mask_to_rows(fake_ctx, None, C.c_int64(0), C.c_int64(0), C.c_int64(8), None, C.c_int64(0), None, None) == 0
    assert lib.vg_mask_to_rows(fake_ctx, None, C.c_int64(0), C.c_int64(1), C.c_int64(8), None, C.c_int64(0), None, None) == -1
    assert b"NULL mask" in lib.vg_last_error()
    byte = (C.c_uint8 * 1)(0xFF)
    assert lib.vg_mask_to_rows(fake_ctx, byte, C.c_int64(0), C.c_int64(2), C.c_int64(8), None, C.c_int64(0), None, None) == -1
    assert b"mask_stride" in lib.vg_last_error()
    assert lib.vg_mask_to_rows(fake_ctx, byte, C.c_int64(0), C.c_int64(1), C.c_int64(1 << 31), None, C.c_int64(0), None, None) == -5
    assert b"2147483648" in lib.vg_last_error()
