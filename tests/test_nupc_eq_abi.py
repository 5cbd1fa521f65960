"""CPU: the non-uniform convolver's equaliser render (bfhip_nupc_reserve_eq / _render_eq_async /
_render_eq, include/bfhip_nupc.h) is exported, bound in Python, and fails cleanly on a NULL handle.
The checks on a live convolver need a device: tests/test_gpu_nupc_eq.py."""
import ctypes as C

import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_reserve_eq", "bfhip_nupc_render_eq_async", "bfhip_nupc_render_eq"]
METHODS = ["reserve_eq", "render_eq_async", "render_eq"]


@pytest.mark.parametrize("name", CALLS)
def test_eq_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


@pytest.mark.parametrize("meth", METHODS)
def test_nupc_binding_has_eq_methods(meth):
    assert callable(getattr(bf.Nupc, meth, None))


def test_eq_calls_fail_on_a_null_handle():
    L = bf.lib()
    freq, mag, phase = (C.c_double * 2)(0.0, 0.5), (C.c_double * 2)(1.0, 1.0), (C.c_double * 2)(0.0, 0.0)
    out = (C.c_float * 8)()
    assert L.bfhip_nupc_reserve_eq(None, 8) < 0
    assert L.bfhip_nupc_render_eq_async(None, 0, 0, 8, 2, freq, mag, phase) < 0
    assert L.bfhip_nupc_render_eq(None, 8, 2, freq, mag, phase, out) < 0
    assert b"null" in L.bfhip_nupc_last_error()
