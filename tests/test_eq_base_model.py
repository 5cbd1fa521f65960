"""CPU: the float64 model of the render onto a base (tests/eq_base_ref.py) that
tests/test_gpu_nupc_eq_base.py holds the device to.  The overlap-save window formula with zero-filled
edges is the truncated convolution, for one partial window, for R not dividing T, for many windows
with a partial last one, and at the largest block length.  This pins the model, not the feature."""
import numpy as np
import pytest

import cases
import eq_base_ref


@pytest.mark.parametrize("T,R,B", [(48, 8, 8), (48, 32, 32), (448, 256, 256), (21760, 64, 2048), (21760, 8192, 8192)])
def test_overlap_save_is_the_truncated_convolution(T, R, B):
    rng = np.random.default_rng(T + R)
    e = rng.standard_normal(R)
    for base in (rng.standard_normal(T), np.concatenate([rng.standard_normal(T - R), np.zeros(R)]), rng.standard_normal(T // 3)):
        want = eq_base_ref.apply(base, e, T)
        assert want.shape == (T,)
        for name, got in (("overlap-save", eq_base_ref.overlap_save(base, e, T, B)), ("one fft", eq_base_ref.apply_fft(base, e, T))):
            err = cases.rel_rms(got, want)
            print("T %d R %d B %d %s: rel rms %.3g (limit 1e-13)" % (T, R, B, name, err))
            assert err <= 1e-13, name


def test_the_convolution_is_truncated_and_trailing_zeros_lose_nothing():
    rng = np.random.default_rng(1)
    T, R = 48, 8
    e = rng.standard_normal(R)
    full = rng.standard_normal(T)
    assert np.array_equal(eq_base_ref.apply(full, e, T), np.convolve(full, e)[:T])
    short = np.concatenate([full[:T - R], np.zeros(R)])
    whole = np.convolve(short[:T - R], e)
    assert len(whole) == T - 1 and cases.rel_rms(eq_base_ref.apply(short, e, T)[:T - 1], whole) <= 1e-15
    pulse = np.zeros(R)
    pulse[R // 2] = 1.0                                     # the linear render of a flat curve: R / 2 frames of delay
    assert np.array_equal(eq_base_ref.apply(full, pulse, T), np.concatenate([np.zeros(R // 2), full[:T - R // 2]]))
