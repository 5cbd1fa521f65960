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


def test_nupc_binding_has_the_format_and_overflow_surface():
    """set_format (gapped frames: the period is L0 frames of sample_spacing * bytes),
    set_safety_limit, and block's overflow[] argument (bfhip_nupc_block's last parameter)"""
    import inspect
    for m in ("set_format", "set_interleaved", "set_safety_limit", "block"):
        assert callable(getattr(bf.Nupc, m, None)), m
    assert "overflow" in inspect.signature(bf.Nupc.block).parameters


def test_nupc_period_sizes_follow_the_frame_layout():
    """the wrapper's period sizes without a device: interleaved frames are n * bytes, gapped
    frames sample_spacing * bytes (set_format / set_interleaved on an object with no handle)"""
    class Stub(bf.Nupc):
        def __init__(self):
            self.h, self.L0, self.n_in, self.n_out = None, 64, 3, 2
            self.in_bytes = self.out_bytes = 0

        def _chk(self, r):
            return 0
    L = bf.lib()
    saved = L.bfhip_nupc_set_format
    try:
        L.bfhip_nupc_set_format = lambda *a: 0
        s = Stub()
        s.set_interleaved(bf.IN, "S24_LE")
        s.set_interleaved(bf.OUT, "S16_LE")
        assert (s.in_bytes, s.out_bytes) == (64 * 3 * 3, 64 * 2 * 2)
        s.set_format(bf.OUT, 0, bf.make_format("S32_LE", 5, 8))
        s.set_format(bf.OUT, 1, bf.make_format("FLOAT_LE", 5, 0))
        assert s.out_bytes == 64 * 5 * 4
    finally:
        L.bfhip_nupc_set_format = saved
