"""CPU: the reservation that lifts the render onto a base beyond 8192 taps
(bfhip_nupc_reserve_eq_base_long, include/bfhip_nupc.h) is exported, bound in Python, and fails cleanly
on a NULL handle.  The checks on a live convolver need a device: tests/test_gpu_nupc_eq_base_long.py."""
import ctypes as C

import brutefir_amd as bf


def test_reserve_eq_base_long_is_exported():
    assert hasattr(C.CDLL(bf.LIB_PATH), "bfhip_nupc_reserve_eq_base_long")


def test_nupc_binding_has_the_method():
    assert callable(getattr(bf.Nupc, "reserve_eq_base_long", None))


def test_reserve_eq_base_long_fails_on_a_null_handle():
    L = bf.lib()
    L.bfhip_nupc_set_format(None, 0, 0, None)                  # leaves another text behind
    assert L.bfhip_nupc_reserve_eq_base_long(None) < 0
    assert b"null" in L.bfhip_nupc_last_error()
