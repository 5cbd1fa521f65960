"""CPU: the run-time control surface of the non-uniform convolver (include/bfhip_nupc.h:
coefficient switches with cross-fade, set rewrites, output gain) is exported, bound in Python,
and every call fails cleanly on a NULL handle.  A convolver needs a device, so the argument
and state checks on a live handle are in tests/test_gpu_nupc_switch.py."""
import ctypes as C

import brutefir_amd as bf

SWITCH_CALLS = ["bfhip_nupc_add_coeff", "bfhip_nupc_set_crossfade", "bfhip_nupc_set_coeff",
                "bfhip_nupc_switch_frame", "bfhip_nupc_switch_busy", "bfhip_nupc_update_coeff",
                "bfhip_nupc_set_output_gain"]


def test_switch_calls_are_exported():
    lib = C.CDLL(bf.LIB_PATH)
    missing = [s for s in SWITCH_CALLS if not hasattr(lib, s)]
    assert not missing, missing


def test_nupc_binding_has_the_switch_methods():
    for m in ("add_coeff", "set_crossfade", "set_coeff", "switch_frame", "switch_busy",
              "update_coeff", "set_output_gain"):
        assert callable(getattr(bf.Nupc, m, None)), m


def test_switch_calls_fail_on_a_null_handle():
    L = bf.lib()
    taps = (C.c_double * 4)()
    assert L.bfhip_nupc_add_coeff(None, 0, taps, 4) < 0
    assert L.bfhip_nupc_set_crossfade(None, 64) < 0
    assert L.bfhip_nupc_set_coeff(None, 0, 1) < 0
    # -1 is "no switch yet": a NULL handle has to be told apart from it
    assert L.bfhip_nupc_switch_frame(None) < -1
    assert L.bfhip_nupc_switch_busy(None) < 0
    assert L.bfhip_nupc_update_coeff(None, 0, 1, taps, 4) < 0
    assert L.bfhip_nupc_set_output_gain(None, 0, 0.5) < 0
