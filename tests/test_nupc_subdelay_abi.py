"""CPU: the sub-sample delay calls of the non-uniform convolver (bfhip_nupc_enable_subdelay /
_set_subdelay / _get_subdelay, include/bfhip_nupc.h) are exported, bound and fail cleanly without
a handle, and bfhip_selftest_subdelay_filter -- the taps the device filters with -- equals the
impulse response of the oracle's sub-sample delay (delay.c:416-505 through its small FFT
overlap-save), so the GPU tests can build their float64 model from the same numbers."""
import ctypes as C

import numpy as np
import pytest

import bforacle as bo
import cases

EINVAL, ESTATE = -1, -5
NAMES = ("bfhip_nupc_enable_subdelay", "bfhip_nupc_set_subdelay", "bfhip_nupc_get_subdelay",
         "bfhip_selftest_subdelay_filter")


def taps_of(bf, half, value, rs):
    out = np.zeros(2 * half + 1, np.float32 if rs == 4 else np.float64)
    assert bf.lib().bfhip_selftest_subdelay_filter(half, value, rs, out.ctypes.data) == 2 * half + 1
    return out


def test_symbols_are_exported_and_bound():
    import brutefir_amd as bf
    raw = C.CDLL(bf.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert getattr(bf.lib(), name).argtypes is not None, name
    for meth in ("enable_subdelay", "set_subdelay", "get_subdelay"):
        assert callable(getattr(bf.Nupc, meth))
    assert bf.UNDEFINED_SUBDELAY == -100


def test_null_handle_fails_cleanly():
    import brutefir_amd as bf
    L = bf.lib()
    assert L.bfhip_nupc_enable_subdelay(None, 31, 9.0) == EINVAL
    assert L.bfhip_nupc_set_subdelay(None, 0, 0, 10) == EINVAL
    assert L.bfhip_nupc_get_subdelay(None, 0, 0) < 0
    assert L.bfhip_nupc_get_subdelay(None, 0, 0) != bf.UNDEFINED_SUBDELAY


def test_selftest_rejects_bad_arguments():
    import brutefir_amd as bf
    L = bf.lib()
    out = np.zeros(64)
    assert L.bfhip_selftest_subdelay_filter(0, 10, 8, out.ctypes.data) == EINVAL
    assert L.bfhip_selftest_subdelay_filter(7, 100, 8, out.ctypes.data) == EINVAL
    assert L.bfhip_selftest_subdelay_filter(7, -100, 8, out.ctypes.data) == EINVAL
    assert L.bfhip_selftest_subdelay_filter(7, 10, 2, out.ctypes.data) == EINVAL
    assert L.bfhip_selftest_subdelay_filter(7, 10, 8, None) == EINVAL


def test_enable_subdelay_argument_checks():
    """the reference's checks and messages (delay.c:458-470) with L0 in the place of the fragment
    size.  They need a handle, and bfhip_nupc_create needs a device to make one: where there is
    none the create call's own error is what can be checked (tests/test_gpu_nupc_subdelay.py runs
    the same checks on the GPU)"""
    import brutefir_amd as bf
    if bf.device_count() == 0:
        with pytest.raises(bf.BfhipError, match="no HIP device"):
            bf.Nupc([64, 128], [2, 2], 4, 1, 1)
        return
    nu = bf.Nupc([64, 128], [2, 2], 4, 1, 1)
    L = bf.lib()
    for half, msg in ((0, b"Invalid half filter length 0."), (-3, b"Invalid half filter length -3."),
                      (32, b"The filter_length must be at least 2 x sdf_length + 1.")):
        assert L.bfhip_nupc_enable_subdelay(nu.h, half, 9.0) == EINVAL
        assert L.bfhip_nupc_last_error() == msg
    nu.close()


@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("half", [7, 15, 31, 128, 255, 511])
def test_value_zero_is_the_unit_pulse(half, rs):
    import brutefir_amd as bf
    want = np.zeros(2 * half + 1)
    want[half] = 1.0
    assert np.array_equal(taps_of(bf, half, 0, rs), want)


@pytest.mark.parametrize("rs,bar", [(4, 1e-5), (8, 1e-12)])
@pytest.mark.parametrize("half", [7, 15, 31, 128, 255, 511])
def test_taps_are_the_oracles_impulse_response(half, rs, bar):
    """a unit pulse through the oracle's engine (dirac filter, `subdelay: v` on the input, the way
    tests/test_oracle_engine.py drives it) is the filter the reference applies; relative RMS at the
    project's parity bars (the oracle goes through its FFT overlap-save: not a bit comparison).
    The half-lengths above 31 are the ones whose filter block size (512, 1024) takes the device's
    FIR through more than one history sample per thread; the oracle engine runs them at the smallest
    block length that admits them, L >= 2 * half + 1."""
    import brutefir_amd as bf
    L = max(64, 1 << (2 * half + 1).bit_length())
    x = np.zeros((L, 1))
    x[0, 0] = 1.0
    for v in (-99, -75, -50, -25, -1, 1, 12, 37, 50, 63, 99):
        e = bo.Engine(L, 1, rs, 1, 1)
        e.set_interleaved(0, "FLOAT64_LE")
        e.set_interleaved(1, "FLOAT64_LE")
        e.enable_subdelay(half)
        e.set_subdelay(0, 0, v)
        e.add_filter(in_ch=[0], out_ch=[0], coeff=-1)
        y = np.concatenate([e.block(b)[1].view(np.float64) for b in (x, np.zeros((L, 1)))])
        got = taps_of(bf, half, v, rs)
        assert cases.rel_rms(got, y[:2 * half + 1]) <= bar, (half, v)
        assert np.abs(y[2 * half + 1:]).max() <= bar, (half, v)
