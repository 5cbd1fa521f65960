"""Float64 model of the minimum-phase equaliser render (bfhip_nupc_render_eq_mode*, mode
BFHIP_EQ_MINIMUM, include/bfhip_nupc.h): the homomorphic method in exactly the header's formulas.

    M[0] = mag[0], M[R/2] = mag[-1], M[n] = ci(mag) at f = n / R          (eq_ref's ci and band search)
    phi[0] = phi[R/2] = 0, phi[n] = ci(phase)
    c     = irfft(log M, R)                                                the real cepstrum
    c^[0] = c[0], c^[t] = 2 c[t] (1 <= t < R/2), c^[R/2] = c[R/2], c^[t] = 0 (t > R/2)
    S     = rfft(c^)
    X[k]  = exp(Re S[k]) / R (cos(Im S[k] + phi[k]) + i sin(Im S[k] + phi[k])),  X[0], X[R/2] real
    taps  = irfft(X, R) * R                                                (the unnormalised HC2R)

Re S[k] = log M[k] in exact arithmetic, so the magnitude response is M, the linear render's.  numpy
and nothing else: no device, no reference tree."""
import numpy as np

import eq_ref


def curve(R, freq, mag, phase):
    """(M, phi) for the bins 0 .. R/2"""
    freq, mag, phase = (np.asarray(v, np.float64) for v in (freq, mag, phase))
    assert R >= 8 and R & (R - 1) == 0 and 2 <= len(freq) == len(mag) == len(phase)
    assert freq[0] == 0.0 and freq[-1] == 0.5 and np.all(np.diff(freq) > 0)
    assert np.all(np.isfinite(mag)) and np.all(mag > 0)
    f = np.arange(1, R // 2) / float(R)
    i = np.searchsorted(freq[1:], f, side="left")           # the first band with f <= freq[i + 1]
    M = np.empty(R // 2 + 1)
    phi = np.zeros(R // 2 + 1)
    M[0], M[-1] = mag[0], mag[-1]
    M[1:-1] = eq_ref.ci(mag[i], mag[i + 1], freq[i], freq[i + 1], f)
    phi[1:-1] = eq_ref.ci(phase[i], phase[i + 1], freq[i], freq[i + 1], f)
    return M, phi


def render(R, freq, mag, phase):
    """R float64 taps: the specification"""
    M, phi = curve(R, freq, mag, phase)
    c = np.fft.irfft(np.log(M), R)
    c[1:R // 2] *= 2.0
    c[R // 2 + 1:] = 0.0
    S = np.fft.rfft(c)
    a = S.imag + phi
    X = np.exp(S.real) / R * (np.cos(a) + 1j * np.sin(a))
    X[0], X[-1] = X[0].real, X[-1].real
    return np.fft.irfft(X, R) * R
