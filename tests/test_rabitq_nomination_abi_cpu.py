"""The RaBitQ batch nomination at the drop-in boundary, without a GPU: the two entry points the header declares are exported by the
library, bound by the Go shim with the declared argument counts, and mirrored in the C++ header and the Python binding; the two
test hooks are known by name — through the helpers of the existing lexical checks (tests/test_go_shim.py, vecgo_amd._lib)."""
from pathlib import Path

from tests import hooks
from tests import test_go_shim as shim
from vecgo_amd import _lib

ROOT = Path(__file__).resolve().parents[1]
NEW = {"vg_index_enable_rabitq_nomination": 3, "vg_index_rabitq_nomination_info": 5}


def test_header_declares_and_library_exports():
    fns, _ = shim.header_functions()
    for name, nargs in NEW.items():
        assert fns.get(name) == nargs, name
    lib, declared = _lib.load(), _lib.declared_symbols()
    for name in NEW:
        assert name in declared and hasattr(lib, name), name
    # a NULL index is a status, not a crash
    assert lib.vg_index_enable_rabitq_nomination(None, 1, None) == -1
    assert lib.vg_index_rabitq_nomination_info(None, None, None, None, None) == -1


def test_go_shim_and_cpp_mirror_bind_them():
    src = (ROOT / "go" / "segment" / "resident.go").read_text()
    calls = dict(shim.c_calls(src))
    for name, nargs in NEW.items():
        assert calls.get(name) == nargs, name
    assert "func (r *Resident) EnableRaBitQNomination(on bool) error" in src
    assert "func (r *Resident) RaBitQNominationInfo() (on bool, heldBytes, rescanned, mismatched int64, err error)" in src
    assert not shim.type_errors({"segment/resident.go": src})
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert "EnableRaBitQNomination" in hpp and "vg_index_enable_rabitq_nomination(h_" in hpp
    assert "RaBitQNominationInfo" in hpp and "vg_index_rabitq_nomination_info(h_" in hpp


def test_python_binding_and_hooks():
    import vecgo_amd
    assert callable(vecgo_amd.Index.enable_rabitq_nomination) and callable(vecgo_amd.Index.rabitq_nomination_info)
    for name in ("VG_RABITQ_NOM_ALWAYS", "VG_RABITQ_NOM_CHECK"):     # an unknown hook name raises
        hooks.set_hook(name, 1)
        hooks.set_hook(name, 0)
