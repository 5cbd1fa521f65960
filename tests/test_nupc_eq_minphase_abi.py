"""CPU: the non-uniform convolver's minimum-phase equaliser render (bfhip_nupc_reserve_eq_minimum /
_render_eq_mode_async / _render_eq_mode, include/bfhip_nupc.h) is exported, bound in Python, and
fails cleanly on a NULL handle.  The checks on a live convolver need a device:
tests/test_gpu_nupc_eq_minphase.py."""
import ctypes as C
import inspect

import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_reserve_eq_minimum", "bfhip_nupc_render_eq_mode_async", "bfhip_nupc_render_eq_mode"]


@pytest.mark.parametrize("name", CALLS)
def test_eq_mode_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


def test_nupc_binding_has_the_reservation_and_the_mode_keyword():
    assert callable(getattr(bf.Nupc, "reserve_eq_minimum", None))
    for meth in ("render_eq", "render_eq_async"):
        mode = inspect.signature(getattr(bf.Nupc, meth)).parameters.get("mode")
        assert mode is not None and mode.default == "linear", meth
    assert (bf.EQ_LINEAR, bf.EQ_MINIMUM) == (0, 1) and bf.EQ_MODES == {"linear": 0, "minimum": 1}


def test_eq_mode_calls_fail_on_a_null_handle():
    L = bf.lib()
    freq, mag, phase = (C.c_double * 2)(0.0, 0.5), (C.c_double * 2)(1.0, 1.0), (C.c_double * 2)(0.0, 0.0)
    out = (C.c_float * 8)()
    for mode in (0, 1):
        for r in (L.bfhip_nupc_reserve_eq_minimum(None),
                  L.bfhip_nupc_render_eq_mode_async(None, 0, 0, 8, 2, freq, mag, phase, mode),
                  L.bfhip_nupc_render_eq_mode(None, 8, 2, freq, mag, phase, mode, out)):
            assert r < 0
            assert b"null" in L.bfhip_nupc_last_error()
