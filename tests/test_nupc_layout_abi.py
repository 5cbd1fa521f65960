"""CPU: the buffer-layout surface of the non-uniform convolver (bfhip_nupc_set_buffer_bytes /
bfhip_nupc_buffer_bytes, include/bfhip_nupc.h) is exported, bound in Python and fails cleanly on
a NULL handle, and brutefir_amd.period_layout lays a side's devices out the way dai.c's
calc_buffer_format does.  The checks on a live handle are in tests/test_gpu_nupc_layouts.py."""
import ctypes as C

import brutefir_amd as bf


def test_layout_calls_are_exported():
    lib = C.CDLL(bf.LIB_PATH)
    missing = [s for s in ("bfhip_nupc_set_buffer_bytes", "bfhip_nupc_buffer_bytes") if not hasattr(lib, s)]
    assert not missing, missing


def test_layout_calls_fail_on_a_null_handle():
    L = bf.lib()
    assert L.bfhip_nupc_set_buffer_bytes(None, bf.IN, 4096) < 0
    assert L.bfhip_nupc_buffer_bytes(None, bf.OUT) < 0


def test_binding_has_the_layout_surface():
    for m in ("set_buffer_bytes", "buffer_bytes"):
        assert callable(getattr(bf.Nupc, m, None)), m
    assert callable(getattr(bf, "period_layout", None))


def test_period_layout_worked_example():
    """L0 = 8.  A: interleaved S16_LE, 3 channels open, selection [2, 0]: 48 bytes, padded to 64.
    B: two FLOAT_LE planes of 32 bytes: 128.  C: one packed S24_LE plane of 24 bytes: 152, padded
    to 160.  Channels are numbered in device order, then selection order."""
    fmts, n_bytes = bf.period_layout(8, [("S16_LE", 3, [2, 0], True),
                                         ("FLOAT_LE", 2, [0, 1], False),
                                         ("S24_LE", 1, [0], False)])
    assert [(f.byte_offset, f.sample_spacing) for f in fmts] == [(4, 3), (0, 3), (64, 1), (96, 1), (128, 1)]
    assert [(f.bytes, f.sbytes, f.isfloat, f.swap) for f in fmts] == [(2, 2, 0, 0)] * 2 + [(4, 4, 1, 0)] * 2 + [(3, 3, 0, 0)]
    assert n_bytes == 160


def test_period_layout_one_planar_device_and_one_interleaved_one():
    """a plane per used channel, not per open one; an interleaved device takes its open channels'
    room whatever is selected; a size that is a multiple of 32 already gets no padding"""
    fmts, n_bytes = bf.period_layout(64, [("S16_LE", 4, [3, 1], False)])
    assert [(f.byte_offset, f.sample_spacing) for f in fmts] == [(0, 1), (128, 1)] and n_bytes == 256
    fmts, n_bytes = bf.period_layout(64, [("S32_LE", 4, [1], True)])
    assert [(f.byte_offset, f.sample_spacing) for f in fmts] == [(4, 4)] and n_bytes == 64 * 4 * 4
    fmts, n_bytes = bf.period_layout(8, [("S24_LE", 1, [0], False)])
    assert n_bytes == 32 and fmts[0].scale == 1.0 / (1 << 23)
