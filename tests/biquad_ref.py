"""Float64 model of the parametric-equaliser sections (bfhip_biquad_design, bfhip_nupc_render_biquads*,
include/bfhip_nupc.h), in exactly the header's formulas.

A section is b0, b1, b2, a1, a2 (a0 = 1).  R = taps, bin n = 0 .. R/2, s = sin^2(pi n / R),
u = sin(2 pi n / R):

    N_k  = ((b0 + b1) + b2) - 2 (b0 + b2) s + i (b0 - b2) u
    D_k  = ((1  + a1) + a2) - 2 (1  + a2) s + i (1  - a2) u
    G[n] = prod_k N_k / D_k                          (k ascending)
    own:     X[n] = G[n] / R,            X[0] = Re G[0] / R,  X[R/2] = Re G[R/2] / R
    linear:  X[n] = (-1)^n |G[n]| / R,   X[0] = |G[0]| / R,   X[R/2] = |G[R/2]| / R
    taps = irfft(X, R) * R                           (the unnormalised HC2R)

impulse() is the independent truth the model itself is held to (tests/test_biquad_model.py): the
plain direct-form recursion.  numpy and nothing else: no device, no reference tree."""
import functools

import numpy as np

PEAK, LOW_SHELF, HIGH_SHELF, LOW_PASS, HIGH_PASS, NOTCH, ALL_PASS = range(7)
OWN, LINEAR = "own", "linear"


def design(type, f0, gain_db, q):
    """the audio-EQ-cookbook section, normalised by a0; 1 - cos w0 and 1 + cos w0 by half angles"""
    assert type in range(7) and 0.0 < f0 < 0.5 and q > 0.0 and np.isfinite(gain_db)
    w0 = 2.0 * np.pi * f0
    c, alpha = np.cos(w0), np.sin(w0) / (2.0 * q)
    S, Cc = np.sin(0.5 * w0) ** 2, np.cos(0.5 * w0) ** 2
    A = 10.0 ** (gain_db / 40.0)
    r = 2.0 * np.sqrt(A) * alpha
    a = [1.0 + alpha, -2.0 * c, 1.0 - alpha]
    if type == PEAK:
        b = [1.0 + alpha * A, -2.0 * c, 1.0 - alpha * A]
        a = [1.0 + alpha / A, -2.0 * c, 1.0 - alpha / A]
    elif type == LOW_SHELF:
        b = [A * ((A + 1.0) - (A - 1.0) * c + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * c), A * ((A + 1.0) - (A - 1.0) * c - r)]
        a = [(A + 1.0) + (A - 1.0) * c + r, -2.0 * ((A - 1.0) + (A + 1.0) * c), (A + 1.0) + (A - 1.0) * c - r]
    elif type == HIGH_SHELF:
        b = [A * ((A + 1.0) + (A - 1.0) * c + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * c), A * ((A + 1.0) + (A - 1.0) * c - r)]
        a = [(A + 1.0) - (A - 1.0) * c + r, 2.0 * ((A - 1.0) - (A + 1.0) * c), (A + 1.0) - (A - 1.0) * c - r]
    elif type == LOW_PASS:
        b = [S, 2.0 * S, S]
    elif type == HIGH_PASS:
        b = [Cc, -2.0 * Cc, Cc]
    elif type == NOTCH:
        b = [1.0, -2.0 * c, 1.0]
    else:
        b = [1.0 - alpha, -2.0 * c, 1.0 + alpha]
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], np.float64)


def stable(sections):
    """the header's section rules: finite, |a2| < 1 and |a1| < 1 + a2"""
    s = np.asarray(sections, np.float64).reshape(-1, 5)
    return bool(1 <= len(s) <= 32 and np.all(np.isfinite(s)) and np.all(np.abs(s[:, 4]) < 1.0)
                and np.all(np.abs(s[:, 3]) < 1.0 + s[:, 4]))


def response(R, sections):
    """G[0 .. R/2], complex128"""
    assert R >= 8 and R & (R - 1) == 0
    n = np.arange(R // 2 + 1)
    s = np.sin(np.pi * n / R) ** 2
    u = np.sin(2.0 * np.pi * n / R)
    G = np.ones(R // 2 + 1, np.complex128)
    for b0, b1, b2, a1, a2 in np.asarray(sections, np.float64).reshape(-1, 5):
        N = ((b0 + b1) + b2) - 2.0 * (b0 + b2) * s + 1j * (b0 - b2) * u
        D = ((1.0 + a1) + a2) - 2.0 * (1.0 + a2) * s + 1j * (1.0 - a2) * u
        G = G * (N / D)
    return G


def render(R, sections, phase=OWN):
    """R float64 taps: the specification"""
    G = response(R, sections)
    if phase == OWN:
        X = G / R
        X[0], X[-1] = X[0].real, X[-1].real
    else:
        assert phase == LINEAR
        n = np.arange(R // 2 + 1)
        X = ((1.0 - 2.0 * (n & 1)) * np.abs(G) / R).astype(np.complex128)
        X[0], X[-1] = abs(G[0]) / R, abs(G[-1]) / R
    return np.fft.irfft(X, R) * R


def impulse(sections, n):
    """the cascade's impulse response h[0 .. n): a plain float64 direct-form recursion, section after section"""
    x = np.zeros(n)
    x[0] = 1.0
    for b0, b1, b2, a1, a2 in np.asarray(sections, np.float64).reshape(-1, 5).tolist():
        y = np.empty(n)
        x1 = x2 = y1 = y2 = 0.0
        for t, xt in enumerate(x.tolist()):
            yt = b0 * xt + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, xt, y1, yt
            y[t] = yt
        x = y
    return x


# ---- section sets the tests share: (n, 5) arrays, read-only

def _ro(rows):
    a = np.array(rows, np.float64).reshape(-1, 5)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sets():
    fs = 48000.0
    rng = np.random.default_rng(2024)
    many = []
    for _ in range(32):
        f0 = float(np.exp(rng.uniform(np.log(0.001), np.log(0.45))))
        many.append(design(int(rng.integers(PEAK, HIGH_SHELF + 1)), f0, float(rng.uniform(-6.0, 6.0)), float(rng.uniform(0.5, 6.0))))
    return {
        "flat": _ro([1.0, 0.0, 0.0, 0.0, 0.0]),
        "tone": _ro([design(LOW_SHELF, 200 / fs, 6.0, 0.707), design(PEAK, 1000 / fs, -4.0, 2.0),
                     design(HIGH_SHELF, 8000 / fs, 3.0, 0.707)]),
        "mixed": _ro([design(PEAK, 0.05, 5.0, 1.5), design(LOW_SHELF, 0.01, -4.0, 0.707), design(HIGH_SHELF, 0.3, 4.0, 0.707),
                      design(LOW_PASS, 0.4, 0.0, 0.9), design(HIGH_PASS, 0.01, 0.0, 0.707), design(NOTCH, 0.1, 0.0, 3.0),
                      design(ALL_PASS, 0.2, 0.0, 1.0)]),
        "room": _ro([design(PEAK, 40 / fs, -9.0, 8.0), design(PEAK, 63 / fs, -6.0, 5.0), design(NOTCH, 50 / fs, 0.0, 30.0),
                     design(HIGH_PASS, 15 / fs, 0.0, 0.707)]),
        "many": _ro(many),
    }
