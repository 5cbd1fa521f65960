"""Float64 model of the equaliser render (bfhip_nupc_render_eq*, include/bfhip_nupc.h): the
reference's render_equaliser (rendereq.h:20-62) for taps = R, in exactly the header's formulas.

    ci(a1, a2, f1, f2, f) = (a1 - a2) 0.5 cos(pi (f - f1) / (f2 - f1)) + (a1 + a2) 0.5
    bin n = 1 .. R/2 - 1:  f = n / R, i the first band with f <= freq[i + 1],
        X[n] = (-1)^n  ci(mag) / R  (cos phi + i sin phi),  phi = ci(phase)
    X[0] = mag[0] / R, X[R/2] = mag[-1] / R
    taps = irfft(X, R) * R                      (the unnormalised HC2R)

render() is the specification (the sign form); render_literal() holds the reference's own
linear-phase term cos(-R pi f + phi), which differs from it by argument rounding only.  numpy and
nothing else: no device, no reference tree."""
import numpy as np


def ci(a1, a2, f1, f2, f):
    return (a1 - a2) * 0.5 * np.cos(np.pi * (f - f1) / (f2 - f1)) + (a1 + a2) * 0.5


def _curve(R, freq, mag, phase):
    """(n, f, m, phi) for the bins 1 .. R/2 - 1"""
    freq, mag, phase = (np.asarray(v, np.float64) for v in (freq, mag, phase))
    assert R >= 8 and R & (R - 1) == 0 and 2 <= len(freq) == len(mag) == len(phase)
    assert freq[0] == 0.0 and freq[-1] == 0.5 and np.all(np.diff(freq) > 0)
    n = np.arange(1, R // 2)
    f = n / float(R)
    i = np.searchsorted(freq[1:], f, side="left")           # the first band with f <= freq[i + 1]
    m = ci(mag[i], mag[i + 1], freq[i], freq[i + 1], f) / R
    phi = ci(phase[i], phase[i + 1], freq[i], freq[i + 1], f)
    return n, f, m, phi, mag


def _taps(R, X_mid, mag):
    X = np.empty(R // 2 + 1, np.complex128)
    X[0], X[-1] = mag[0] / R, mag[-1] / R
    X[1:-1] = X_mid
    return np.fft.irfft(X, R) * R


def render(R, freq, mag, phase):
    """R float64 taps: the specification"""
    n, f, m, phi, mag = _curve(R, freq, mag, phase)
    sign = 1.0 - 2.0 * (n & 1)
    return _taps(R, sign * m * (np.cos(phi) + 1j * np.sin(phi)), mag)


def render_literal(R, freq, mag, phase):
    """the same with the reference's literal linear-phase term: re = cos(-R pi f + phi) m, im = sin(...) m"""
    n, f, m, phi, mag = _curve(R, freq, mag, phase)
    arg = -(R * np.pi) * f + phi
    return _taps(R, m * (np.cos(arg) + 1j * np.sin(arg)), mag)


# ---- curves the tests share (freq, mag, phase)

def flat():
    return [0.0, 0.5], [1.0, 1.0], [0.0, 0.0]


def random_bands(n_bands, seed, db=12.0):
    """n_bands knots, magnitudes within +-db dB, phases in (-3, 3)"""
    rng = np.random.default_rng(seed)
    inner = np.sort(rng.uniform(0.0005, 0.4995, n_bands - 2))
    assert np.all(np.diff(inner) > 0)
    freq = np.concatenate([[0.0], inner, [0.5]])
    mag = 10.0 ** (rng.uniform(-db, db, n_bands) / 20.0)
    phase = rng.uniform(-3.0, 3.0, n_bands)
    return list(freq), list(mag), list(phase)


def knot_on_a_bin():
    """knots at 5/64 and 0.25: bin frequencies of every length from 64 up (5/64 from 64, 0.25 from 8)"""
    return [0.0, 5.0 / 64, 0.25, 0.5], [1.0, 2.0, 0.5, 1.5], [0.0, 1.0, -2.0, 0.5]


def skipped_band():
    """two knots less than one bin apart at R = 64 (between bins 6 and 7): no bin falls into that band"""
    return [0.0, 6.3 / 64, 6.6 / 64, 0.5], [1.0, 3.0, 0.25, 1.0], [0.5, -1.0, 2.0, 0.0]
