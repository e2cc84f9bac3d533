"""The SQ8 nomination from the codes at the drop-in boundary, without a GPU: the two entry points the header declares are exported
by the library, bound by the Go shim with the declared argument counts, and mirrored in the C++ header — through the helpers of
the existing lexical checks (tests/test_go_shim.py, vecgo_amd._lib)."""
from pathlib import Path

from tests import test_go_shim as shim
from vecgo_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
NEW = {"vg_index_enable_sq8_nomination_from_codes": 3, "vg_index_sq8_nomination_info": 4}


def test_header_declares_and_library_exports():
    fns, _ = shim.header_functions()
    for name, nargs in NEW.items():
        assert fns.get(name) == nargs, name
    lib, declared = _lib.load(), _lib.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(lib, name), name
    # a NULL index is a status, not a crash
    assert lib.vg_index_enable_sq8_nomination_from_codes(None, 1, None) == -1
    assert lib.vg_index_sq8_nomination_info(None, None, None, None) == -1


def test_go_shim_and_cpp_mirror_bind_them():
    src = (ROOT / "go" / "segment" / "resident.go").read_text()
    calls = dict(shim.c_calls(src))
    for name, nargs in NEW.items():
        assert calls.get(name) == nargs, name
    assert "func (r *Resident) EnableSQ8NominationFromCodes(on bool) error" in src
    assert "func (r *Resident) SQ8NominationInfo() (mode int, heldBytes, rescanned int64, err error)" in src
    assert not shim.type_errors({"segment/resident.go": src})
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert "EnableSQ8NominationFromCodes" in hpp and "vg_index_enable_sq8_nomination_from_codes(h_" in hpp
    assert "SQ8NominationInfo" in hpp and "vg_index_sq8_nomination_info(h_" in hpp


def test_python_binding_has_the_methods():
    import vecgo_amd
    assert callable(vecgo_amd.Index.enable_sq8_nomination_from_codes) and callable(vecgo_amd.Index.sq8_nomination_info)
