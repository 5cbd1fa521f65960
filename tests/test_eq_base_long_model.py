"""CPU: the float64 model that tests/test_gpu_nupc_eq_base_long.py holds the long render onto a base to
(eq_taps > 8192 under bfhip_nupc_reserve_eq_base_long; tests/eq_base_ref.py).  At these lengths the
device's block is B = R, and the truth is the one float64 FFT of the whole length, never the direct sum:
overlap-save with B = R is that FFT's result for two windows with a partial second one, for one whole
window, and at the first length that needs more than one combine pass of the big FFT.  Measured here:
at most 5.8e-16 relative RMS (T = 21760), 0 where T = R (one window: the same transform length as the
one FFT).  This pins the model, not the feature."""
import numpy as np
import pytest

import cases
import eq_base_ref


@pytest.mark.parametrize("T,R", [(21760, 16384), (16384, 16384), (131072, 131072)])
def test_overlap_save_with_one_block_per_curve_length_is_the_truncated_convolution(T, R):
    rng = np.random.default_rng(T + R)
    e = rng.standard_normal(R)
    for base in (rng.standard_normal(T), np.concatenate([rng.standard_normal(T - R), np.zeros(R)]), rng.standard_normal(T // 3)):
        want = eq_base_ref.apply_fft(base, e, T)
        got = eq_base_ref.overlap_save(base, e, T, B=R)
        assert want.shape == got.shape == (T,) and np.any(want) == np.any(base)   # T = R: the second base is all zeros
        err = cases.rel_rms(got, want)
        print("T %d R %d B %d: rel rms %.3g (limit 1e-13)" % (T, R, R, err))
        assert err <= 1e-13


def test_the_one_fft_is_the_direct_sum_where_both_can_be_had():
    """apply_fft is the truth of the long lengths: at a length where the direct sum is still quick they agree"""
    rng = np.random.default_rng(3)
    T, R = 4096, 1024
    base, e = rng.standard_normal(T), rng.standard_normal(R)
    assert cases.rel_rms(eq_base_ref.apply_fft(base, e, T), eq_base_ref.apply(base, e, T)) <= 1e-13
