"""copra_batch_set_cost_weights at the C ABI: declared, exported, and the ABI version that has it (no GPU needed)."""
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


def test_set_cost_weights_is_exported_with_abi_6():
    lib = _lib()
    assert hasattr(lib, "copra_batch_set_cost_weights")
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 6


def test_header_declares_set_cost_weights():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    assert "copra_status_t copra_batch_set_cost_weights(copra_batch_t* h, int cost_index, const double* w, int on_device);" in text


def test_python_binding_has_set_cost_weights():
    from copra_amd import BatchLMPC
    assert callable(getattr(BatchLMPC, "set_cost_weights", None))
