"""The SQ8 nomination from the codes for small batches at the drop-in boundary, without a GPU: on = 2 of
vg_index_enable_sq8_nomination_from_codes needs no new symbol — the Go shim, the C++ mirror and the Python binding name it, and the
ABI minor stands — through the helpers of the existing lexical checks (tests/test_go_shim.py)."""
import inspect
from pathlib import Path

from tests import test_go_shim as shim

ROOT = Path(__file__).resolve().parents[1]


def test_go_shim_and_cpp_mirror_name_the_small_batches():
    src = (ROOT / "go" / "segment" / "resident.go").read_text()
    assert "func (r *Resident) EnableSQ8NominationFromCodesSmallBatches() error" in src
    assert "C.vg_index_enable_sq8_nomination_from_codes(r.h, C.int32_t(2), nil)" in src
    assert dict(shim.c_calls(src)).get("vg_index_enable_sq8_nomination_from_codes") == 3
    assert not shim.type_errors({"segment/resident.go": src})
    hpp = (ROOT / "include" / "vecgo_hip.hpp").read_text()
    assert "EnableSQ8NominationFromCodesSmallBatches" in hpp and "vg_index_enable_sq8_nomination_from_codes(h_, 2, nullptr)" in hpp


def test_python_binding_takes_small_batches_and_the_abi_minor_stands():
    import vecgo_amd
    assert "small_batches" in inspect.signature(vecgo_amd.Index.enable_sq8_nomination_from_codes).parameters
    assert "#define VG_ABI_MINOR 13\n" in (ROOT / "include" / "vecgo_hip.h").read_text()
