"""Float64 model of the look-ahead peak limiter on the non-uniform convolver's outputs
(include/bfhip_nupc.h), for the tests.  numpy only: no device.

    envelope   s from p by the definition, term by term: the release recursion walks the frames one
               by one, the window minimum and the box sum walk j = 0 .. D (newest frame first)
    limit      a [frames][n_out] array of x through groups with by-period thresholds: D frames of
               delay on every channel, grouped channels times their group's s in the real type
    LimitedChain   nupc_chain_ref.Chain with the limiter in front of nupc_ref.encode"""
import numpy as np

import nupc_chain_ref as cr
import nupc_ref as nr


def release_coef(release):
    return 0.0 if release == 0 else float(np.exp(-1.0 / release))


def envelope_parts(p, D, release):
    """(r, m, e, s) of the definition from p[0..n), fresh state"""
    p = np.asarray(p, np.float64)
    n = len(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(p > 1.0, 1.0 / p, 1.0)
    rp = np.concatenate([np.ones(D), r])
    m = rp[D:].copy()
    for j in range(1, D + 1):
        m = np.minimum(m, rp[D - j:D - j + n])
    a = release_coef(release)
    e = np.ones(D + n)                                # e[t < 0] = 1 in front
    prev = 1.0
    ml = m.tolist()
    out = [0.0] * n
    for t in range(n):
        rel = 1.0 - a * (1.0 - prev)
        prev = ml[t] if ml[t] < rel else rel
        out[t] = prev
    e[D:] = out
    acc = np.zeros(n)
    for j in range(D + 1):
        acc = acc + e[D - j:D - j + n]
    return r, m, e[D:], acc / float(D + 1)


def envelope(p, D, release):
    return envelope_parts(p, D, release)[3]


def delayed(x, D):
    """x[t - D], x[t < 0] = 0, along axis 0"""
    x = np.asarray(x)
    return np.concatenate([np.zeros((D,) + x.shape[1:], x.dtype), x[:len(x) - D]])


def peaks(x, chs, ceil):
    """p[t] = max over the group's channels of |x| / ceil (ceil: [frames][len(chs)] or [len(chs)]);
    a non-finite x counts as 0"""
    v = np.asarray(x, np.float64)[:, list(chs)]
    with np.errstate(invalid="ignore"):
        q = np.where(np.isfinite(v), np.abs(v) / ceil, 0.0)
    return q.max(axis=1)


def by_frame(thr, periods, L0):
    """a threshold, or one per period, as one per frame"""
    t = np.asarray(thr, np.float64)
    return np.repeat(np.full(periods, t) if t.ndim == 0 else t, L0)


def limit(x, groups, scales, D, release, L0, dt=np.float64):
    """x: [frames][n_out] float64 in output units; groups: [(channels, threshold or [per period])];
    scales: fmt.scale per channel.  Returns (y [frames][n_out] float64, [s per group])."""
    x = np.asarray(x, np.float64)
    n = len(x)
    xd = delayed(x, D)
    y = xd.copy()
    env = []
    for chs, thr in groups:
        ceil = by_frame(thr, n // L0, L0)[:, None] / np.array([scales[c] for c in chs], np.float64)[None, :]
        s = envelope(peaks(x, chs, ceil), D, release)
        env.append(s)
        for c in chs:
            with np.errstate(invalid="ignore", over="ignore"):
                y[:, c] = (xd[:, c].astype(dt) * s.astype(dt)).astype(np.float64)
    return y, env


class LimitedChain(cr.Chain):
    """Chain with bfhip_nupc_enable_limiter: render() limits the reals in front of nupc_ref.encode,
    with y / scale as the limiter's x, thresholds by period and D frames of delay on every output."""

    def limiter(self, D, release):
        self.lim_D, self.lim_release, self.lim_groups = D, release, []

    def group(self, chs, thr):
        self.lim_groups.append((tuple(chs), thr))
        return len(self.lim_groups) - 1

    def set_threshold(self, p, g, thr):
        self._ev(p, "thr", g, thr)

    def _thr(self, g, periods):
        v, out = self.lim_groups[g][1], []
        for p in range(periods):
            for kind, a in self.events.get(p, ()):
                if kind == "thr" and a[0] == g:
                    v = a[1]
            out.append(v)
        return out

    def render(self, x_raw, periods, frames=None):
        # Chain.render has no step to hook into in front of encode, so this is its body (input side, segment
        # outputs, blend, gains, output sub-delay FIR, resets, encode, output side) with limit() between the
        # FIR and encode; the division by scale there is done for every run here, since the limiter's x is in
        # output units.  A change to Chain.render has to be repeated here.
        n, L0 = periods * self.L0, self.L0
        x = self.inputs(x_raw, periods)
        start = [(0, 1.0)] * len(self.filters)
        ys = [self.yseg(x, start)] + [self.yseg(x, a) for _, _, _, a in self.commits]
        y = cr.blend(ys, [(t, m, F, k + 1) for k, (t, m, F, _) in enumerate(self.commits)], self.sched, frames)
        y = y * self.gains(periods)
        scale = np.array([f.scale for f in self.fmts[cr.OUT]])
        y = y / scale
        for ch in self.sub0[cr.OUT]:
            y[:, ch] = cr.fir(y[:, ch], self._vals(cr.OUT, ch, periods), self.half, self.rs, L0)
        groups = [(chs, self._thr(g, periods)) for g, (chs, _) in enumerate(self.lim_groups)]
        y, self.env = limit(y, groups, scale, self.lim_D, self.lim_release, L0)
        y = y * scale
        resets = [p for p in range(periods) if any(k == "reset" for k, _ in self.events.get(p, ()))]
        raw, of, status = nr.encode(y, self.fmts[cr.OUT], L0, dither=self.dither, rate=self.rate, resets=resets)
        return cr.Result(self._side(cr.OUT, raw, periods), of, status, y)
