"""CPU: the non-uniform convolver's equaliser render onto a base impulse response
(bfhip_nupc_reserve_eq_base / _set_eq_base / _render_eq_base_async / _render_eq_base,
include/bfhip_nupc.h) is exported, bound in Python, and fails cleanly on a NULL handle.  The checks on
a live convolver need a device: tests/test_gpu_nupc_eq_base.py."""
import ctypes as C
import inspect

import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_reserve_eq_base", "bfhip_nupc_set_eq_base", "bfhip_nupc_render_eq_base_async", "bfhip_nupc_render_eq_base"]


@pytest.mark.parametrize("name", CALLS)
def test_eq_base_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


def test_nupc_binding_has_the_four_methods():
    for meth in ("reserve_eq_base", "set_eq_base", "render_eq_base_async", "render_eq_base"):
        assert callable(getattr(bf.Nupc, meth, None)), meth
    for meth in ("render_eq_base_async", "render_eq_base"):
        mode = inspect.signature(getattr(bf.Nupc, meth)).parameters.get("mode")
        assert mode is not None and mode.default == "linear", meth


def test_eq_base_calls_fail_on_a_null_handle():
    L = bf.lib()
    freq, mag, phase = (C.c_double * 2)(0.0, 0.5), (C.c_double * 2)(1.0, 1.0), (C.c_double * 2)(0.0, 0.0)
    out = (C.c_float * 8)()
    for call in (lambda: L.bfhip_nupc_reserve_eq_base(None, 0),
                 lambda: L.bfhip_nupc_set_eq_base(None, 0, out, 8),
                 lambda: L.bfhip_nupc_render_eq_base_async(None, 0, 0, 8, 2, freq, mag, phase, 0),
                 lambda: L.bfhip_nupc_render_eq_base_async(None, 0, 0, 8, 2, freq, mag, phase, 1),
                 lambda: L.bfhip_nupc_render_eq_base(None, 0, 8, 2, freq, mag, phase, 0, out),
                 lambda: L.bfhip_nupc_render_eq_base(None, 0, 8, 2, freq, mag, phase, 1, out)):
        L.bfhip_nupc_set_format(None, 0, 0, None)              # leaves another text behind
        assert call() < 0
        assert b"null" in L.bfhip_nupc_last_error()
