"""No-GPU checks of vg_bm25_update's restatement (tests/bm25_update_ref.py): pinned against tests/bm25_ref.py's MemoryIndex over a
random script of adds, deletes and replaces in batches, with freed doc ids reused as the reference reuses them; the host-side
refusals against the plain-Python statement of the same rules; and the header / binding surface of the new entry points."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tests import bm25_ref as ref
from tests import bm25_update_ref as uref

ROOT = Path(__file__).resolve().parents[1]
NEW = ["vg_bm25_create_empty", "vg_bm25_update", "vg_bm25_export"]
QUERIES = ["w0", "w1 w3", "w0 w2 w5 w9", "w39 w17", "w7 w7", "nothing"]


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def apply_batch(drv, csr, batch):
    for op in batch:
        drv.add(op[1], op[2]) if op[0] == "add" else drv.delete(op[1])
    a = drv.flush()
    return a, uref.update(csr, a["del_docs"], a["add_docs"], a["add_len"], a["add_off"], a["add_terms"], a["add_tf"], a["n_docs"], a["n_terms"],
                          a["add_ids"])


def check_searches(drv, csr, a, k=7):
    for text in QUERIES:
        want = drv.mem.search(text, k, sort=True)
        terms, idfs = drv.query(text)
        if a["doc_count"] == 0:
            assert want == []
            continue
        ids, sc, n = ref.csr_search(csr.term_off, csr.post_doc, csr.post_tf, csr.doc_len, a["total_length"], a["doc_count"], terms, idfs, k, csr.doc_to_id)
        assert n == len(want) and ids[:n].tolist() == [pk for pk, _ in want], (text, ids, want)
        assert np.array_equal(bits(sc[:n]), bits([s for _, s in want])), text


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_follows_the_memory_index(seed):
    drv, csr = uref.Driver(), uref.Csr(mapped=True)
    reused = replaced = emptied = 0
    for batch in uref.zipf_script(seed, 400):
        free_before = set(drv.mem.free_ids)
        a, csr = apply_batch(drv, csr, batch)
        reused += len(free_before & set(a["add_docs"].tolist()))
        replaced += len(set(a["del_docs"].tolist()) & set(a["add_docs"].tolist()))
        emptied += a["doc_count"] == 0
        assert drv.lists_equal(csr)
        for t in range(csr.n_terms):                                  # strictly ascending lists
            li = csr.post_doc[csr.term_off[t]:csr.term_off[t + 1]]
            assert np.all(li[1:] > li[:-1])
        check_searches(drv, csr, a)
    assert reused > 0 and replaced > 0 and emptied == 1 and drv.mem.doc_count > 0   # the script covers what it is for


def test_term_ids_are_stable_and_sizes_never_shrink():
    csr = uref.Csr()
    csr = uref.update(csr, None, [0, 1], [2, 1], [0, 2, 3], [0, 1, 1], [1, 1, 1], 2, 2)
    assert csr.term_off.tolist() == [0, 1, 3] and csr.post_doc.tolist() == [0, 0, 1]
    gone = uref.update(csr, [0], None, None, None, None, None, 2, 4)                # term 0 empties, terms 2 and 3 are unused new ids
    assert gone.term_off.tolist() == [0, 0, 1, 1, 1] and gone.post_doc.tolist() == [1] and gone.doc_len.tolist() == [0, 1]
    again = uref.update(gone, None, [0], [1], [0, 1], [3], [5], 2, 4)               # the freed id is reused, in a new term
    assert again.term_off.tolist() == [0, 0, 1, 1, 2] and again.post_doc.tolist() == [1, 0] and again.post_tf.tolist() == [1, 5]
    for bad in (dict(n_docs_new=1, n_terms_new=4), dict(n_docs_new=2, n_terms_new=3)):
        with pytest.raises(uref.Refused):
            uref.update(again, None, None, None, None, None, None, **bad)


def test_host_side_refusals_name_the_doc_or_term():
    csr = uref.update(uref.Csr(), None, [0, 1], [1, 1], [0, 1, 2], [0, 0], [1, 1], 2, 1)
    cases = [
        ("doc named twice", 3, dict(add_docs=[3, 3], add_off=[0, 1, 2], add_terms=[0, 0])),
        ("term named twice", 1, dict(add_docs=[2], add_off=[0, 2], add_terms=[1, 1])),
        ("added doc out of range", 9, dict(add_docs=[9], add_off=[0, 1], add_terms=[0])),
        ("deleted doc out of range", 2, dict(del_docs=[2])),
        ("term out of range", 5, dict(add_docs=[2], add_off=[0, 1], add_terms=[5])),
        ("add into a live slot", 1, dict(add_docs=[1], add_off=[0, 1], add_terms=[0])),
    ]
    for what, number, kw in cases:
        n = len(kw.get("add_docs", []))
        with pytest.raises(uref.Refused) as e:
            uref.update(csr, kw.get("del_docs"), kw.get("add_docs"), [1] * n, kw.get("add_off"), kw.get("add_terms"),
                        [1] * len(kw.get("add_terms", [])), 4, 2)
        assert e.value.what == what and e.value.number == number
    ok = uref.update(csr, [1], [1], [3], [0, 1], [0], [2], 4, 2)                        # the same add as a replace is fine
    assert ok.post_doc.tolist() == [0, 1] and ok.post_tf.tolist() == [1, 2] and ok.doc_len.tolist() == [1, 3, 0, 0]


def test_header_binding_and_exports_name_the_new_entry_points():
    from vecgo_amd import _lib
    import vecgo_amd as vg
    text = (ROOT / "include" / "vecgo_hip.h").read_text()
    assert re.search(r"#define VG_ABI_MINOR 13\b", text)
    note = text[text.index("Added at minor 13 without a bump"):text.index("#define VG_ABI_MINOR")]
    assert "vg_bm25_create_empty, vg_bm25_update" in note and "vg_bm25_export, found by symbol lookup" in note
    lib = _lib.load()
    go = (ROOT / "go" / "lexical" / "bm25_hip.go").read_text()
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    api = (ROOT / "vecgo_amd" / "api.py").read_text()
    for name in NEW:
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        assert f"{name}(" in hpp and f"_lib.{name}" in api, name
    assert "C.vg_bm25_update(" in go and "C.vg_bm25_create_empty(" in go
    assert int(re.search(r"#define VG_BM25_UPDATE_CHUNK (\d+)", text).group(1)) == vg.BM25_UPDATE_CHUNK
    assert "BM25_UPDATE_CHUNK" in vg.__all__
    for cite in ("bm25.go:238-278", ":180-229", ":191-195", ":259-261", "FAILURE IS ATOMIC", "STABLE TERM IDS", "NOT TESTED"):
        assert cite in text, cite
    wait = text[text.index("These WAIT for"):text.index("Entry points in neither list")]
    assert "vg_bm25_update" in wait


def test_malformed_calls_are_refused_without_a_device():
    from vecgo_amd import _lib
    lib = _lib.load()
    z = C.c_int64(0)
    assert lib.vg_bm25_create_empty(None, 0, None) == -1
    assert lib.vg_bm25_update(None, None, z, None, None, None, z, None, None, None, z, z, z, z, None) == -1
    assert lib.vg_bm25_export(None, None, None, None, None, None, None) == -1
