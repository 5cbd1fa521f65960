"""CPU: per-filter gains, the ramped output gain and the peak reset of the non-uniform convolver
(include/bfhip_nupc.h) are exported, bound in Python, and every call fails cleanly on a NULL
handle.  A convolver needs a device, so the argument and state checks on a live handle are in
tests/test_gpu_nupc_gain.py."""
import ctypes as C
import math

import brutefir_amd as bf

GAIN_CALLS = ["bfhip_nupc_reserve_filter_gain", "bfhip_nupc_set_filter_gain", "bfhip_nupc_get_filter_gain",
              "bfhip_nupc_set_gain_ramp", "bfhip_nupc_reset_overflow"]


def test_gain_calls_are_exported():
    lib = C.CDLL(bf.LIB_PATH)
    missing = [s for s in GAIN_CALLS if not hasattr(lib, s)]
    assert not missing, missing


def test_nupc_binding_has_the_gain_methods():
    for m in ("reserve_filter_gain", "set_filter_gain", "get_filter_gain", "set_gain_ramp", "reset_overflow"):
        assert callable(getattr(bf.Nupc, m, None)), m


def test_gain_calls_fail_on_a_null_handle():
    L = bf.lib()
    assert L.bfhip_nupc_reserve_filter_gain(None) < 0
    assert L.bfhip_nupc_set_filter_gain(None, 0, 0.5) < 0
    assert math.isnan(L.bfhip_nupc_get_filter_gain(None, 0))
    assert L.bfhip_nupc_set_gain_ramp(None, 64) < 0
    assert L.bfhip_nupc_reset_overflow(None) < 0
