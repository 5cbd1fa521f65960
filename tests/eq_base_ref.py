"""The float64 model of the equaliser render onto a base impulse response (bfhip_nupc_render_eq_base*,
include/bfhip_nupc.h; brutefir_amd/csrc/eq_apply.h).

    y[t] = sum_{j = 0}^{min(t, R - 1)} e[j] b[t - j],   0 <= t < T

e: the R rendered taps (tests/eq_ref.py, tests/eq_minphase_ref.py), b: the base of at most T taps,
zero-padded.  The convolution is truncated at T."""
import numpy as np


def apply(base, e, T):
    """the truncated convolution, summed directly in float64"""
    b = np.zeros(T)
    b[:min(len(base), T)] = np.asarray(base, np.float64)[:T]
    return np.convolve(b, np.asarray(e, np.float64))[:T]


def apply_fft(base, e, T):
    """the same by one float64 FFT of the whole length: for lengths at which the direct sum takes minutes"""
    b = np.zeros(T)
    b[:min(len(base), T)] = np.asarray(base, np.float64)[:T]
    n = 1 << int(np.ceil(np.log2(T + len(e))))
    return np.fft.irfft(np.fft.rfft(b, n) * np.fft.rfft(np.asarray(e, np.float64), n), n)[:T]


def overlap_save(base, e, T, B):
    """what the device computes: window j of ceil(T / B) is b[(j - 1) B, (j + 1) B) with zeros in front of
    tap 0 and behind T; the last B values of its circular convolution with e, zero-padded to 2B, are
    y[j B, (j + 1) B)"""
    R = len(e)
    assert R <= B
    b = np.zeros(T)
    b[:min(len(base), T)] = np.asarray(base, np.float64)[:T]
    E = np.fft.rfft(np.asarray(e, np.float64), 2 * B)
    n_win = (T + B - 1) // B
    padded = np.concatenate([np.zeros(B), b, np.zeros((n_win + 1) * B - T)])
    y = np.zeros(n_win * B)
    for j in range(n_win):
        w = padded[j * B:(j + 2) * B]                      # b[(j - 1) B, (j + 1) B)
        y[j * B:(j + 1) * B] = np.fft.irfft(np.fft.rfft(w) * E, 2 * B)[B:]
    return y[:T]
