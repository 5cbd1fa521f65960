"""CPU: HP-TPDF dither on the non-uniform convolver's outputs (bfhip_nupc_enable_dither,
include/bfhip_nupc.h) is exported, bound in Python, and fails cleanly on a NULL handle.  The
checks on a live convolver need a device: tests/test_gpu_nupc_dither.py."""
import ctypes as C

import brutefir_amd as bf


def test_enable_dither_is_exported():
    assert hasattr(C.CDLL(bf.LIB_PATH), "bfhip_nupc_enable_dither")


def test_nupc_binding_has_enable_dither():
    assert callable(getattr(bf.Nupc, "enable_dither", None))


def test_enable_dither_fails_on_a_null_handle():
    chs = (C.c_int * 2)(0, 1)
    assert bf.lib().bfhip_nupc_enable_dither(None, chs, 2, 48000, 0) < 0
