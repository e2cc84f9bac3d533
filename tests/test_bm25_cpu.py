"""No-GPU checks of hybrid search: tests/bm25_ref.py (lexical/bm25 MemoryIndex and the RRF loop restated) pinned against the
reference's own test inputs (tests/golden/bm25_kats.json), the tie behaviour vg_bm25_search reproduces, the stated deviation
about unsorted posting lists, and the header / binding / Go surface of the new entry points."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import bm25_ref as ref

ROOT = Path(__file__).resolve().parents[1]
NEW = ["vg_bm25_create", "vg_bm25_destroy", "vg_bm25_stats", "vg_bm25_search", "vg_bm25_replayed", "vg_rrf_fuse"]


@pytest.fixture(scope="module")
def kats(golden_dir):
    return json.loads((golden_dir / "bm25_kats.json").read_text())


def expect(res, want):
    ids = [pk for pk, _ in res]
    if "len" in want:
        assert len(res) == want["len"], (ids, want)
    if "first" in want:
        assert ids[0] == want["first"], (ids, want)
    for pk in want.get("contains", []):
        assert pk in ids, (ids, want)
    assert all(s > 0 for _, s in res)
    assert all(res[i][1] >= res[i + 1][1] for i in range(len(res) - 1))


@pytest.mark.parametrize("name", ["Basic", "Delete", "MultiTerm", "Heap_Logic", "DeleteEfficiency", "Unicode"])
def test_reference_known_answers(kats, name):
    mem = ref.MemoryIndex()
    for step in kats["bm25"][name]:
        if step[0] == "add":
            mem.add(step[1], step[2])
        elif step[0] == "add_range":
            for i in range(step[1], step[2]):
                mem.add(i, step[3])
        elif step[0] == "delete":
            mem.delete(step[1])
        else:
            expect(mem.search(step[1], step[2]), step[3])
            expect(mem.search(step[1], step[2], sort=True), step[3])   # the shim's sorted lists answer the same


def test_reference_hybrid_known_answers(kats):
    h = kats["hybrid"]
    mem = ref.MemoryIndex()
    vec = {}
    for r in h["rows"]:
        mem.add(r["id"], r["text"])
        vec[r["id"]] = np.asarray(r["vector"], np.float32)
    for s in h["searches"]:
        q = np.asarray(s["vector"], np.float32)
        vk = max(2 * s["k"], 50)
        by_dist = sorted(vec, key=lambda pk: (float(np.sum((vec[pk] - q) ** 2, dtype=np.float32)), pk))[:vk]
        lex = [pk for pk, _ in mem.search(s["text"], vk)]
        ids, sc, n = ref.rrf_fuse(by_dist, lex, s["rrf_k"], s["k"])
        if "first" in s["expect"]:
            assert ids[0] == s["expect"]["first"]
        for pk in s["expect"].get("contains", []):
            assert pk in ids[:n].tolist()


def test_the_constants_are_the_references():
    """k1 + 1, k1 * (1 - b) and k1 * b are exact constant expressions in Go, rounded once; float64 arithmetic on 1.2 would not
    always give the same double — which is why the library and the restatement spell them out"""
    assert ref.K1_PLUS_1 == 2.2 and ref.K1_1B == 0.3 and ref.K1_B == 0.9
    assert 1.2 * 0.75 != 0.9 or 1.2 * (1 - 0.75) != 0.3 or 1.2 + 1 != 2.2   # at least one differs when computed in float64
    src = (ROOT / "vecgo_amd" / "csrc" / "k_bm25.hip").read_text()
    for lit in ("= 2.2;", "= 0.3;", "= 0.9 / avg_dl;"):
        assert lit in src, lit


def test_tie_example_answers_c_b():
    """k = 2, scores 1, 1, 2 in doc order: the heap is [A, B], C replaces the root A, the answer is [C, B] — ordering by
    (score desc, doc asc) would say [C, A]"""
    one, two = np.float32(1), np.float32(2)
    assert ref.heap_topk([(one, "A"), (one, "B"), (two, "C")], 2) == [("C", two), ("B", one)]
    mem = ref.MemoryIndex()
    mem.add(10, "x y")          # A
    mem.add(11, "x z")          # B: same tf, same length: the same score bits
    mem.add(12, "x x")          # C: tf 2
    res = mem.search("x", 2)
    assert [pk for pk, _ in res] == [12, 11] and res[0][1] > res[1][1]


def test_risk_rule_by_brute_force():
    """What vg_bm25_search's fast path rests on: when the best min(hits, k + 1) scores are pairwise different among the first
    k and the (k + 1)-th lies strictly below the k-th, the heap's answer is the sort's — whatever ties lie below."""
    rng = np.random.default_rng(4)
    checked = 0
    for _ in range(3000):
        n, k = int(rng.integers(1, 14)), int(rng.integers(1, 8))
        scores = rng.integers(1, 9, n).astype(np.float32)          # few values: ties are everywhere
        order = sorted(range(n), key=lambda i: (-scores[i], i))
        top = [scores[i] for i in order[:k + 1]]
        distinct = all(top[i] > top[i + 1] for i in range(min(len(top), k) - 1))
        below = len(top) <= k or top[k] < top[k - 1]
        got = ref.heap_topk([(float(scores[i]), i) for i in range(n)], k)
        if distinct and below:
            assert got == [(i, scores[i]) for i in order[:k]], (scores, k)
            checked += 1
        else:
            assert sorted(s for _, s in got) == sorted(scores[i] for i in order[:k])   # the scores agree, the docs need not
    assert checked > 300


def test_unsorted_list_scores_a_doc_in_pieces():
    """The stated deviation: after a swap-remove and the reuse of a freed doc id the reference's posting list is out of order,
    and its document-at-a-time walk meets a doc twice — each time with a part of its score.  The shim sorts the lists."""
    mem = ref.MemoryIndex()
    mem.add(1, "y")             # doc 0
    mem.add(2, "x y")           # doc 1
    mem.add(3, "x y y")         # doc 2
    mem.delete(1)               # the swap-remove moves y's last posting to the front: y = [2, 1], while x = [1, 2]
    assert [d for d, _ in mem.inverted["y"]] == [2, 1] and [d for d, _ in mem.inverted["x"]] == [1, 2]
    lists, idfs = mem.iterators("x y")
    walk = ref.daat_scores(lists, idfs, mem.doc_lengths, mem.total_length, mem.doc_count)
    assert [d for d, _ in walk] == [1, 2, 1]                            # doc 1 is met twice: scored in pieces
    sorted_lists, _ = mem.iterators("x y", sort=True)
    walk_sorted = ref.daat_scores(sorted_lists, idfs, mem.doc_lengths, mem.total_length, mem.doc_count)
    assert [d for d, _ in walk_sorted] == [1, 2]
    assert [pk for pk, _ in mem.search("x y", 10)].count(2) == 2        # ... and reported twice, each time with a part
    whole = dict(walk_sorted)
    pieces = {}
    for d, s in walk:
        pieces.setdefault(d, []).append(s)
    twice = [d for d in pieces if len(pieces[d]) == 2]
    assert twice and all(max(pieces[d]) < whole[d] for d in twice)      # each piece is less than the doc's score
    header = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert "STRICTLY ASCENDING doc order" in header and "swap-remove" in header and "NOT validated" in header


def test_rrf_restatement():
    ids, sc, n = ref.rrf_fuse([7, 3, 7], [3, 9], 60, 5)
    f = np.float32
    assert n == 3 and ids[:3].tolist() == [3, 9, 7]
    assert sc[0] == f(f(1) / f(62)) + f(1) / f(61) and sc[1] == f(1) / f(62) and sc[2] == f(1) / f(63)   # 7 keeps its LAST rank
    ids, sc, n = ref.rrf_fuse([5], [6], 0, 2)
    assert ids.tolist() == [5, 6] and sc[0] == sc[1] == f(1)           # equal scores: ascending id


def test_header_declares_exports_and_notes_the_new_entry_points():
    from vecgo_amd import _lib
    import vecgo_amd as vg
    text = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR 13\b", text)
    note = text[text.index("Added at minor 13 without a bump"):text.index("#define VG_ABI_MINOR")]
    lib = _lib.load()
    assert "vg_bm25_create / _destroy / _stats / _search / _replayed" in note and "vg_rrf_fuse, found by symbol lookup" in note
    for name in NEW:
        assert name in _lib.declared_symbols(), name
        assert hasattr(lib, name), f"libvecgo_hip.so does not export {name}"
    assert int(re.search(r"#define VG_BM25_TILE_DOCS (\d+)", text).group(1)) == vg.BM25_TILE_DOCS
    for cite in ("engine.go:1538-1640", "bm25.go:282-381", "bm25.go:314-317", ":394-441", "engine.go:1560-1602", "ASCENDING ID"):
        assert cite in text, cite
    enqueue = text[text.index("Enqueue-only entry points"):text.index("These WAIT for")]
    wait = text[text.index("These WAIT for"):text.index("Entry points in neither list")]
    assert "vg_rrf_fuse" in enqueue and "vg_bm25_search" in wait and "vg_bm25_search" not in enqueue


def test_bindings_name_the_new_surface():
    import vecgo_amd as vg
    go = (ROOT / "go" / "lexical" / "bm25_hip.go").read_text()
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    api = (ROOT / "vecgo_amd" / "api.py").read_text()
    for name in NEW:
        assert f"C.{name}(" in go, name
        assert f"{name}(" in hpp, name
        assert f"_lib.{name}" in api, name
    assert go.startswith("//go:build hip && cgo\n") and "var _ Index = (*HipIndex)(nil)" in go
    for method in ("Add(id model.ID, text string) error", "Delete(id model.ID) error",
                   "Search(ctx context.Context, text string, k int) ([]model.Candidate, error)", "Close() error"):
        assert f"func (x *HipIndex) {method}" in go, method
    assert "math.Log(1+(n-df+0.5)/(df+0.5))" in go and "sort.Slice" in go and "x.dirty" in go
    for name in ("Bm25", "rrf_fuse", "hybrid_search", "BM25_TILE_DOCS"):
        assert name in vg.__all__ and hasattr(vg, name), name


def test_malformed_calls_are_refused_without_a_device():
    """every refusal here comes before the library touches a device"""
    from vecgo_amd import _lib
    lib = _lib.load()
    assert lib.vg_bm25_search(None, None, None, None, C.c_int64(1), 1, None, None, None, None) == -1
    assert lib.vg_bm25_create(None, C.c_int64(1), C.c_int64(1), None, None, None, None, C.c_int64(1), C.c_int64(1), None, None) == -1
    assert lib.vg_rrf_fuse(None, C.c_int64(1), None, None, C.c_int64(0), None, None, C.c_int64(0), 60, 1, None, None, None, None) == -1
    assert lib.vg_bm25_destroy(None) == 0
    assert lib.vg_bm25_replayed(None, None, None) == -1 and lib.vg_bm25_stats(None, None, None, None, None) == -1
