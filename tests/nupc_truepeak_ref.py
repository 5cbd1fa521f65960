"""Float64 model of the limiter's true-peak detector (include/bfhip_nupc.h, "true-peak detection for the
limiter"), for the tests.  numpy only: no device.

    taps       g[q - 1][k], q = 1 .. 3, k = 0 .. 2 H - 1: Kaiser-windowed sinc, beta = 8, I0 by its power series
    phases     u[t][q], q = 0 .. 3, of one channel: u_0[t] = x~[t - H], u_q[t] = sum over k ascending of
               g_q[k] x~[t - k], with x~ = x where finite, else 0, and x~[t < 0] = 0
    detect     max over q of |u[t][q]|
    limit_tp   nupc_limiter_ref.limit with this detector: the envelope looks ahead D_e = D - H frames, every
               channel is still D frames late.  Also returns each group's true-peak reading by frame
    LimitedChainTP   nupc_limiter_ref.LimitedChain in true-peak mode"""
import numpy as np

import nupc_limiter_ref as lr

H = 12
BETA = 8.0
SAMPLE_PEAK, TRUE_PEAK = 0, 1


def i0(x):
    """sum of ((x / 2)^k / k!)^2: all terms positive"""
    h, term, total = 0.5 * x, 1.0, 1.0
    for k in range(1, 200):
        term *= (h / k) * (h / k)
        total += term
        if term < total * 1e-17:
            break
    return total


def taps():
    g = np.zeros((3, 2 * H))
    for q in (1, 2, 3):
        for k in range(2 * H):
            v = k - H + q / 4.0
            g[q - 1, k] = np.sin(np.pi * v) / (np.pi * v) * i0(BETA * np.sqrt(1.0 - (v / H) ** 2)) / i0(BETA)
    return g


G = taps()


def phases(x):
    """[n][4] from one channel x[0..n)"""
    x = np.asarray(x, np.float64)
    n = len(x)
    xt = np.concatenate([np.zeros(2 * H - 1), np.where(np.isfinite(x), x, 0.0)])      # x~[t] in cell t + 2 H - 1
    u = np.zeros((n, 4))
    u[:, 0] = xt[H - 1:H - 1 + n]
    for q in range(3):
        acc = np.zeros(n)
        for k in range(2 * H):
            acc = acc + G[q, k] * xt[2 * H - 1 - k:2 * H - 1 - k + n]
        u[:, q + 1] = acc
    return u


def detect(x):
    return np.abs(phases(x)).max(axis=1)


def peaks_tp(x, chs, ceil):
    """p[t] = max over the group's channels and the four phases of |u| / ceil (ceil as in lr.peaks)"""
    tp = np.stack([detect(np.asarray(x, np.float64)[:, c]) for c in chs], axis=1)
    return (tp / ceil).max(axis=1)


def limit_tp(x, groups, scales, D, release, L0, dt=np.float64):
    """lr.limit in true-peak mode -> (y [frames][n_out], [s per group], [true peak per group and frame, as a
    fraction of full scale: max over members and phases of |u| * scale])"""
    assert D >= 2 * H
    x = np.asarray(x, np.float64)
    n = len(x)
    xd = lr.delayed(x, D)
    y = xd.copy()
    env, meter = [], []
    for chs, thr in groups:
        sc = np.array([scales[c] for c in chs], np.float64)
        ceil = lr.by_frame(thr, n // L0, L0)[:, None] / sc[None, :]
        s = lr.envelope(peaks_tp(x, chs, ceil), D - H, release)
        env.append(s)
        meter.append((np.stack([detect(x[:, c]) for c in chs], axis=1) * sc[None, :]).max(axis=1))
        for c in chs:
            with np.errstate(invalid="ignore", over="ignore"):
                y[:, c] = (xd[:, c].astype(dt) * s.astype(dt)).astype(np.float64)
    return y, env, meter


class LimitedChainTP(lr.LimitedChain):
    """LimitedChain with bfhip_nupc_set_limiter_detector(TRUE_PEAK): render() calls lr.limit, which this class
    swaps for limit_tp while it runs"""

    def render(self, x_raw, periods, frames=None):
        def limit(y, groups, scale, D, release, L0):
            out, env, self.true_peak = limit_tp(y, groups, scale, D, release, L0)
            return out, env

        keep, lr.limit = lr.limit, limit
        try:
            return super().render(x_raw, periods, frames)
        finally:
            lr.limit = keep
