"""CPU: the non-uniform convolver's asynchronous set rewrite (bfhip_nupc_reserve_update /
_update_buffer / _update_coeff_async / _update_coeff_dev_async / _update_busy / _update_result /
_update_wait, include/bfhip_nupc.h) is exported, bound in Python, and fails cleanly on a NULL
handle.  The checks on a live convolver need a device: tests/test_gpu_nupc_rewrite.py."""
import ctypes as C

import pytest

import brutefir_amd as bf

CALLS = ["bfhip_nupc_reserve_update", "bfhip_nupc_update_buffer", "bfhip_nupc_update_coeff_async",
         "bfhip_nupc_update_coeff_dev_async", "bfhip_nupc_update_busy", "bfhip_nupc_update_result",
         "bfhip_nupc_update_wait"]
METHODS = ["reserve_update", "update_buffer", "update_coeff_async", "update_coeff_dev_async", "update_busy",
           "update_result", "update_wait"]


@pytest.mark.parametrize("name", CALLS)
def test_rewrite_calls_are_exported(name):
    assert hasattr(C.CDLL(bf.LIB_PATH), name)


@pytest.mark.parametrize("meth", METHODS)
def test_nupc_binding_has_rewrite_methods(meth):
    assert callable(getattr(bf.Nupc, meth, None))


def test_rewrite_calls_fail_on_a_null_handle():
    L = bf.lib()
    taps = (C.c_float * 4)(1, 2, 3, 4)
    assert L.bfhip_nupc_reserve_update(None) < 0
    assert L.bfhip_nupc_update_buffer(None) is None
    assert L.bfhip_nupc_update_coeff_async(None, 0, 0, taps, 4) < 0
    assert L.bfhip_nupc_update_coeff_dev_async(None, 0, 0, taps, 4, None) < 0
    assert L.bfhip_nupc_update_busy(None) < 0
    assert L.bfhip_nupc_update_result(None) < 0
    assert L.bfhip_nupc_update_wait(None) < 0
    assert b"null" in L.bfhip_nupc_last_error()

