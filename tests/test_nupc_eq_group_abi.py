"""CPU: the group render of the non-uniform convolver (bfhip_nupc_reserve_eq_group / _render_eq_group_async /
_update_result_member, include/bfhip_nupc.h) is exported, bound in Python, and fails cleanly on a NULL
handle; where a device is there, the reservation's order and size checks.  The checks on a live convolver
need a device: tests/test_gpu_nupc_eq_group.py."""
import ctypes as C
import inspect
import os
import re

import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_reserve_eq_group", "bfhip_nupc_render_eq_group_async", "bfhip_nupc_update_result_member"]
EINVAL, ESTATE = -1, -5
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bfhip_nupc.h")


@pytest.mark.parametrize("name", CALLS)
def test_group_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


@pytest.mark.parametrize("name", CALLS)
def test_group_calls_are_declared(name):
    text = open(HEADER).read()
    assert re.search(r"\bint %s\(bfhip_nupc \*n," % name, text), name
    assert re.search(r"#define BFHIP_NUPC_GROUP_MAX 16\b", text)


def test_nupc_binding_has_the_three_methods():
    for meth in ("reserve_eq_group", "render_eq_group_async", "update_result_member"):
        assert callable(getattr(bf.Nupc, meth, None)), meth
    par = inspect.signature(bf.Nupc.render_eq_group_async).parameters
    assert list(par)[1:9] == ["filters", "coeffs", "onto_base", "eq_taps", "freq", "mag", "phase", "mode"]
    assert par["mode"].default == "linear"


def test_group_calls_fail_on_a_null_handle():
    L = bf.lib()
    freq, mag, phase = (C.c_double * 2)(0.0, 0.5), (C.c_double * 2)(1.0, 1.0), (C.c_double * 2)(0.0, 0.0)
    two = (C.c_int * 2)(0, 1)
    for call in (lambda: L.bfhip_nupc_reserve_eq_group(None, 4),
                 lambda: L.bfhip_nupc_render_eq_group_async(None, 2, two, two, two, 8, 2, freq, mag, phase, 0),
                 lambda: L.bfhip_nupc_render_eq_group_async(None, 2, two, two, None, 8, 2, freq, mag, phase, 1),
                 lambda: L.bfhip_nupc_update_result_member(None, 0)):
        L.bfhip_nupc_set_format(None, 0, 0, None)              # leaves another text behind
        assert call() == EINVAL
        assert b"null" in L.bfhip_nupc_last_error()


def test_reservation_order_and_sizes():
    """they need a handle, and bfhip_nupc_create needs a device to make one: where there is none the create
    call's own error is what can be checked (tests/test_gpu_nupc_eq_group.py runs the same checks on the GPU)"""
    if bf.device_count() == 0:
        with pytest.raises(bf.BfhipError, match="no HIP device"):
            bf.Nupc([8, 16], [2, 2], 4, 1, 1)
        return
    L = bf.lib()
    nu = bf.Nupc([8, 16], [2, 2], 4, 1, 1)
    assert L.bfhip_nupc_reserve_eq_group(nu.h, 4) == ESTATE      # before reserve_eq
    assert b"reserve_eq" in L.bfhip_nupc_last_error()
    nu.reserve_update()
    nu.reserve_eq(32)
    for size in (-1, 0, 1, 17):
        assert L.bfhip_nupc_reserve_eq_group(nu.h, size) == EINVAL, size
    nu.reserve_eq_group(2)
    nu.reserve_eq_group(16)
    assert L.bfhip_nupc_update_result_member(nu.h, 0) == ESTATE  # before finalize
    nu.close()
