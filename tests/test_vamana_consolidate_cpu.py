"""vg_vamana_consolidate without a GPU: the symbol is exported and declared with its argument list, the minor version is
unchanged, the C++ / Go / Python mirrors name the call; the sequential restatement (tests/vamana_consolidate_ref.py) holds
the invariants the header states, its batch schedule changes the graph, and it passes the reference's Delete test."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import vamana_consolidate_ref as ref
from tests import vamana_fresh_ref as fresh

ROOT = Path(__file__).resolve().parents[1]


def _header_and_minor():
    h = (ROOT / "include" / "vecgo_hip.h").read_text()
    return h, h[h.index("Added at minor 13 without a bump"):h.index("#define VG_ABI_MINOR")]


def test_symbol_is_exported_and_refuses_a_null_index():
    from vecgo_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "vg_vamana_consolidate")
    assert lib.vg_abi_minor() == 13
    stats = (C.c_int64 * 4)(7, 7, 7, 7)
    st = lib.vg_vamana_consolidate(None, 100, C.c_float(1.2), None, 8192, stats, None)
    assert st == -1 and b"NULL index" in lib.vg_last_error()
    assert list(stats) == [7, 7, 7, 7]  # written only on VG_OK


def test_header_declares_the_arguments_and_the_stats():
    h, minor = _header_and_minor()
    decl = re.search(r"int32_t vg_vamana_consolidate\(([^)]*)\);", h)
    assert decl
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["vg_index *idx", "int32_t l", "float alpha", "const uint8_t *deleted", "int32_t max_batch",
                    "vg_vamana_consolidate_stats *stats", "void *stream"]
    body = re.search(r"typedef struct vg_vamana_consolidate_stats \{(.*?)\} vg_vamana_consolidate_stats;", h, flags=re.S).group(1)
    assert re.findall(r"int64_t (\w+);", body) == list(ref.STAT_NAMES)
    assert "vg_vamana_consolidate" in minor  # found by symbol lookup until the next bump
    assert "#define VG_ABI_MINOR 13" in h


def test_mirrors_name_the_call():
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert re.search(r"vg_vamana_consolidate_stats ConsolidateVamana\(const uint8_t \*deleted, int l = 100, float alpha = 1\.2f, "
                     r"int maxBatch = 8192\)", hpp)
    assert "vg_vamana_consolidate(h_, l, alpha, deleted, maxBatch, &stats, nullptr)" in hpp
    go = (ROOT / "go" / "segment" / "resident.go").read_text()
    assert "func (r *Resident) ConsolidateVamana(" in go and "C.vg_vamana_consolidate(" in go
    body = go[go.index("func (r *Resident) ConsolidateVamana("):]
    body = body[:body.index("\n}\n")]
    assert "(r.rows+7)/8" in body  # the length check InsertVamana makes


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_python_wrapper_checks_its_arguments_first():
    from vecgo_amd import api
    idx = api.Index.__new__(api.Index)
    idx._lib, idx._h, idx.n, idx.dim = _NoLibrary(), None, 300, 16
    with pytest.raises(ValueError, match="300"):
        idx.consolidate_vamana(np.zeros(299, bool))
    with pytest.raises(ValueError, match="38"):
        idx.consolidate_vamana(np.zeros(37, np.uint8))  # packed: ceil(300 / 8) = 38 bytes
    with pytest.raises(ValueError, match="1024"):
        idx.consolidate_vamana(np.zeros(300, bool), l=1025)
    with pytest.raises(ValueError, match="16384"):
        idx.consolidate_vamana(np.zeros(300, bool), max_batch=16385)
    with pytest.raises(ValueError, match="16384"):
        idx.consolidate_vamana(np.zeros(300, bool), max_batch=0)
    with pytest.raises(TypeError):
        idx.consolidate_vamana(np.zeros(300, bool), l=20.0)
    with pytest.raises(TypeError):
        idx.consolidate_vamana(np.zeros(300, bool), max_batch="8")
    with pytest.raises(TypeError):
        idx.consolidate_vamana(np.zeros(300, bool), alpha="1.2")


# ---- the restatement's invariants ------------------------------------------------------------------------
def _recount(before, after, deleted, repaired):
    return {"repaired_nodes": len(repaired), "dropped_links": sum(int(deleted[v]) for i in repaired for v in before[i]),
            "links_before": sum(len(before[i]) for i in repaired), "links_after": sum(len(after[i]) for i in repaired)}


@pytest.mark.parametrize("max_batch", ref.SCHEDULE_BATCHES)
def test_restatement_invariants(max_batch):
    base, deleted, before, entry, after, stats, repaired = ref.schedule_case(max_batch)
    n = len(before)
    assert 40 < deleted.sum() < 80  # about 20 %
    assert repaired == sorted(repaired) and repaired == [i for i in range(n) if not deleted[i] and any(deleted[v] for v in before[i])]
    assert len(repaired) > 50
    for i in range(n):
        if deleted[i] or i not in set(repaired):
            assert after[i] == before[i], i  # deleted nodes' lists and the untouched live lists
        if not deleted[i]:
            assert not any(deleted[v] for v in after[i]), i  # no live node lists a deleted node
        assert len(after[i]) <= 8 and len(set(after[i])) == len(after[i]) and i not in after[i], i
        assert all(0 <= v < n for v in after[i]), i
    assert stats == _recount(before, after, deleted, repaired)
    assert stats["dropped_links"] >= stats["repaired_nodes"] and stats["links_after"] > 0
    # a second run with the same bitmap repairs nothing and changes nothing
    again, stats2, repaired2 = ref.consolidate(base, after, entry, 8, l=20, deleted=deleted, max_batch=max_batch)
    assert again == after and repaired2 == [] and stats2 == ref.ZERO_STATS
    # the table form: repaired rows are dense prefixes, the others keep their bits
    arr = ref.expected_array(fresh.array_of(before, 8), after, repaired, 8)
    assert fresh.lists_of(arr) == after
    assert not ((arr[:, :-1] == ref.INVALID) & (arr[:, 1:] != ref.INVALID)).any()


def test_nothing_deleted_is_a_no_op():
    base, deleted, before, entry = ref.schedule_case()
    for d in (None, np.zeros(300, bool)):
        after, stats, repaired = ref.consolidate(base, before, entry, 8, l=20, deleted=d, max_batch=32)
        assert after == before and repaired == [] and stats == ref.ZERO_STATS


def test_the_schedule_matters():
    """The serial loop and the batched runs leave different graphs on this input (SCHEDULE_DATA_SEED): a batch's later nodes
    do not see its earlier nodes' new lists."""
    runs = {mb: ref.schedule_case(mb) for mb in ref.SCHEDULE_BATCHES}
    assert runs[1][6] == runs[32][6] == runs[16384][6]  # the same repair set
    differ = lambda a, b: sum(x != y for x, y in zip(runs[a][4], runs[b][4]))
    d32, dall, dboth = differ(1, 32), differ(1, 16384), differ(32, 16384)
    print(f"lists that differ: max_batch 1 vs 32: {d32}, 1 vs 16384: {dall}, 32 vs 16384: {dboth}")
    assert d32 > 0 and dall > 0 and dboth > 0


# ---- the reference's Delete test ---------------------------------------------------------------------------
def test_reference_delete_shape():
    """fresh_vamana_test.go:71-116 with a consolidate before the search: 10 rows, none of them deleted."""
    base, deleted, before, entry = ref.delete_test_case()
    after, stats, repaired = ref.consolidate(base, before, entry, fresh.DEFAULT_R, deleted=deleted)
    assert stats["repaired_nodes"] == len(repaired) > 0 and all(i >= 50 for i in repaired)
    assert not any(v < 50 for i in range(50, 100) for v in after[i])
    ids, scores, counts = fresh.search(base, after, entry, base[:1], 10, deleted=deleted)
    assert counts[0] == 10 and ids[0].min() >= 50 and len(set(ids[0].tolist())) == 10
    print(f"repaired {len(repaired)}; search for row 0 returns ids {ids[0].tolist()}")


@pytest.mark.parametrize("live", [(17, 60), (60,)])
def test_degenerate_all_but_two_and_all_but_one(live):
    base, _, before, entry = ref.delete_test_case()
    deleted = np.ones(100, bool)
    deleted[list(live)] = False
    after, stats, repaired = ref.consolidate(base, before, entry, fresh.DEFAULT_R, deleted=deleted)
    assert repaired == sorted(live)  # a default-option list of 99 other rows always names a deleted one
    if len(live) == 2:
        assert after[live[0]] == [live[1]] and after[live[1]] == [live[0]]  # each reaches the other through deleted nodes
        assert stats["links_after"] == 2
    else:
        assert after[live[0]] == [] and stats["links_after"] == 0
    assert all(after[i] == before[i] for i in range(100) if deleted[i])
