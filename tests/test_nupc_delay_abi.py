"""CPU: per-channel integer delay and mute on the non-uniform convolver's raw I/O blocks
(bfhip_nupc_set_maxdelay / _set_delay / _set_mute / _get_delay, include/bfhip_nupc.h) are
exported, bound in Python, and fail cleanly on a NULL handle.  The checks on a live convolver
need a device: tests/test_gpu_nupc_delay.py."""
import ctypes as C

import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_set_maxdelay", "bfhip_nupc_set_delay", "bfhip_nupc_set_mute", "bfhip_nupc_get_delay"]


@pytest.mark.parametrize("name", CALLS)
def test_delay_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


@pytest.mark.parametrize("meth", ["set_maxdelay", "set_delay", "set_mute", "get_delay"])
def test_nupc_binding_has_delay_methods(meth):
    assert callable(getattr(bf.Nupc, meth, None))


def test_delay_calls_fail_on_a_null_handle():
    L = bf.lib()
    for io in (bf.IN, bf.OUT):
        assert L.bfhip_nupc_set_maxdelay(None, io, 0, 100) < 0
        assert L.bfhip_nupc_set_delay(None, io, 0, 10) < 0
        assert L.bfhip_nupc_set_mute(None, io, 0, 1) < 0
        assert L.bfhip_nupc_get_delay(None, io, 0) < 0
