"""Float64 model of the whole per-period chain of the non-uniform convolver (include/bfhip_nupc.h),
for the tests.  numpy, the oracle library and bfhip_selftest_subdelay_filter only: no device.

The convolver runs every run-time control in one chain per period of L0 frames:

    input    mute -> raw delay line -> raw to real -> sub-delay FIR
    middle   per-segment convolutions under one or two assignments, blended per segment (staggered
             switch) or over their sum (aligned switch)
    output   x gain(frame) / scale -> sub-delay FIR -> quantise or dither -> raw delay line -> mute

and this module holds one piece per step, each the one the per-feature tests use:

    Line / Model   the oracle's integer delay (bfo_delay_new / bfo_delay_update) per raw channel with
                   the channel's mute in dai.c's order: input mute before the line, output mute
                   behind it.  Fragment (L0) and sample size are parameters.
    taps / fir     the sub-delay FIR per period on the unfiltered history, from the taps the library
                   reports
    blend          a list of commits (t_req, mode, F, assignment) over per-segment outputs:
                   nupc_stagger_ref.staggered / nupc_ref.switched
    GainRamp       the output gain record of nupc_sched.h as a [frames][n_out] array
    nupc_ref.encode  per period, with dither, overflow structs and status

Chain composes them; session() draws the event lists of the session tests."""
import ctypes as C
import hashlib

import numpy as np

import bforacle as bo
import nupc_ref as nr
import nupc_stagger_ref as sr

IN, OUT = 0, 1
ALIGNED, STAGGERED = 0, 1


# ---------------------------------------------------------------- raw delay and mute

def _olib():
    L = bo.lib()
    L.bfo_delay_new.restype = C.c_void_p
    L.bfo_delay_new.argtypes = [C.c_int] * 4
    L.bfo_delay_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.bfo_delay_free.argtypes = [C.c_void_p]
    return L


class Line:
    """the oracle's delay line of one raw channel (fragment L0, nbytes per sample) and the
    channel's mute, with the order dai.c uses on the side.  init 0 with maxd <= 0 is no line."""

    def __init__(self, io, init, maxd, nbytes, L0):
        self.io, self.ss, self.maxd, self.L0 = io, nbytes, maxd, L0
        self.d = _olib().bfo_delay_new(L0, init, maxd, nbytes) if (init or maxd > 0) else None
        self.req, self.muted = init, False
        self.cur = 0 if maxd == 0 else init          # curdelay (tests keep init <= a positive maxd)

    def __del__(self):
        if self.d:
            _olib().bfo_delay_free(self.d)

    def run(self, frames, ch):
        """frames: [L0][frame bytes] uint8, modified in place; the channel's samples lie at byte
        ch * nbytes of every frame"""
        s = np.ascontiguousarray(frames[:, ch * self.ss:(ch + 1) * self.ss])
        if self.io == IN and self.muted:
            s[:] = 0
        if self.d:
            _olib().bfo_delay_update(self.d, s.ctypes.data, int(self.req))
            if self.req != self.cur and self.req <= self.maxd:
                self.cur = self.req
        if self.io == OUT and self.muted:
            s[:] = 0
        frames[:, ch * self.ss:(ch + 1) * self.ss] = s


class Model:
    """the lines of one side with interleaved frames of one sample format"""

    def __init__(self, io, fmt, spec, L0):
        """spec: per channel (initial delay, maxdelay)"""
        self.nbytes, self.L0 = bo.SAMPLE_FORMATS[fmt][0], L0
        self.lines = [Line(io, d, m, self.nbytes, L0) for d, m in spec]

    def run(self, raw):
        fr = np.ascontiguousarray(raw).view(np.uint8).reshape(self.L0, -1).copy()
        for ch, ln in enumerate(self.lines):
            ln.run(fr, ch)
        return fr.ravel()


# ---------------------------------------------------------------- sub-sample delay

_TAPS = {}


def taps(half, v, rs):
    """the device's taps for value v, as float64 (computed once per key)"""
    import brutefir_amd as bf
    key = (half, v, rs)
    if key not in _TAPS:
        out = np.zeros(2 * half + 1, np.float32 if rs == 4 else np.float64)
        assert bf.lib().bfhip_selftest_subdelay_filter(half, v, rs, out.ctypes.data) == 2 * half + 1
        _TAPS[key] = out.astype(np.float64)
    return _TAPS[key]


def fir(x, vals, half, rs, L0):
    """the stream x (float64 [frames]) through the per-period filters: period p uses the taps of
    vals[p] from its first frame on, on the unfiltered history; x[t < 0] = 0.  vals None: the
    channel has no filter and is delayed by `half` whole frames."""
    n = len(x)
    pad = np.concatenate([np.zeros(2 * half), x])
    if vals is None:
        return pad[half:half + n].copy()
    y = np.zeros(n)
    for p in range(n // L0):
        seg = pad[p * L0:(p + 1) * L0 + 2 * half]
        y[p * L0:(p + 1) * L0] = np.convolve(seg, taps(half, vals[p], rs), mode="valid")
    return y


# ---------------------------------------------------------------- switches

def aligned_frame(sched, t_req):
    """t_sw of an aligned switch committed at t_req: the header's max over the segments"""
    return max([t_req] + sr.switch_frames(sched, t_req))


def blend(yseg, commits, sched, frames=None):
    """yseg[a]: [segment][frames][n_out] under assignment a (0: the one the run starts with);
    commits: [(t_req, mode, F, a)] in order, at distinct t_req.  An aligned commit switches every
    segment at aligned_frame, a staggered one each segment at its own t_k.  frames(t_req) -> [t_k]
    replaces the staggered formula.  Returns [frames][n_out]."""
    if all(mode == ALIGNED for _, mode, _, _ in commits):
        return nr.switched([np.asarray(y).sum(axis=0) for y in yseg],
                           [(aligned_frame(sched, t), F, a) for t, _, F, a in commits])
    n_seg = len(sched[0])
    frames = frames or (lambda t_req: sr.switch_frames(sched, t_req))
    t_k = {t: (frames(t) if mode == STAGGERED else [aligned_frame(sched, t)] * n_seg) for t, mode, _, _ in commits}
    assert len(t_k) == len(commits)
    return sr.staggered(yseg, [(t, F, a) for t, _, F, a in commits], sched, frames=lambda t: t_k[t])


# ---------------------------------------------------------------- output gain

class GainRamp:
    """the per-frame output gain g[frames][n_out] by the record of nupc_sched.h: from the first
    frame of the period a target was set in, frame idx has gain a + (g - a)(idx + 1) / len below
    len - 1, then g; a is the gain of the last emitted frame.  len 0 is a step."""

    def __init__(self, n_frames, L0, g0):
        self.L0, self.g0 = L0, list(g0)
        self.g = np.ones((n_frames, len(g0))) * np.array(g0, np.float64)
        self.tgt, self.R, self.pend = list(g0), 0, {}

    def set_ramp(self, R):
        self.R = R

    def request(self, ch, g):
        """set_output_gain: of several calls before one block call the last counts; a call with
        the value already asked for changes nothing (and keeps the earlier call's ramp length)"""
        if g != self.pend.get(ch, (self.tgt[ch],))[0]:
            self.pend[ch] = (g, self.R)

    def commit(self, b):
        """the block call of period b takes the pending targets"""
        t0, n = b * self.L0, len(self.g)
        for ch, (g, R) in self.pend.items():
            if g == self.tgt[ch]:
                continue
            a = self.g[t0 - 1, ch] if t0 else self.g0[ch]
            j = np.arange(n - t0)
            self.g[t0:, ch] = g if R == 0 else np.where(j >= R - 1, g, a + (g - a) * ((j + 1) / float(max(R, 1))))
            self.tgt[ch] = g
        self.pend = {}


# ---------------------------------------------------------------- the chain

def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a, np.float64).tobytes()).digest()


class Result:
    def __init__(self, raw, overflow, status, reals):
        self.raw, self.overflow, self.status, self.reals = raw, overflow, status, reals


class Chain:
    """One convolver's configuration, the calls made on it (each with the period whose block call
    it precedes) and the expected output.  Interleaved frames of one format per side.  filter f
    holds versions h[f][v] of taps; sets[f][s] is the version set s holds now."""

    def __init__(self, sched, rs, n_in, n_out, infmt, outfmt, half=None, dither=(), rate=300, cache=None):
        self.sched, self.rs, self.n_in, self.n_out = sched, rs, n_in, n_out
        self.L0 = sched[0][0]
        self.taps = sum(L * N for L, N in zip(*sched))
        self.names = (infmt, outfmt)
        self.fmts = (bo.interleaved_formats(infmt, n_in), bo.interleaved_formats(outfmt, n_out))
        self.half, self.dither, self.rate = half, tuple(dither), rate
        self.filters, self.h, self.hd, self.sets = [], [], [], []
        self.delay = ({}, {})                     # side -> {ch: (init, maxd)}
        self.sub0 = ({}, {})                      # side -> {ch: initial value}
        self.events = {}                          # period -> [(kind, args)]
        self.commits = []                         # (t_req, mode, F, assignment)
        self.asg = []
        self.cur_delay = {}                       # side -> the delays in force after render()
        self._y = {} if cache is None else cache

    # ---- configuration
    def add_filter(self, i, o, sets, in_scale=1.0, out_scale=1.0):
        self.filters.append((i, o, in_scale, out_scale))
        self.h.append([np.asarray(h, np.float64) for h in sets])
        self.hd.append([_digest(h) for h in self.h[-1]])
        self.sets.append(list(range(len(sets))))
        self.asg.append((0, 1.0))
        return len(self.filters) - 1

    def line(self, io, ch, init, maxd):
        self.delay[io][ch] = (init, maxd)

    def subdelay(self, io, ch, v):
        self.sub0[io][ch] = v

    # ---- calls in front of block call p
    def _ev(self, p, kind, *args):
        self.events.setdefault(p, []).append((kind, args))

    def set_delay(self, p, io, ch, d):
        self._ev(p, "delay", io, ch, d)

    def set_mute(self, p, io, ch, m):
        self._ev(p, "mute", io, ch, bool(m))

    def set_subdelay(self, p, io, ch, v):
        self._ev(p, "sub", io, ch, v)

    def set_gain(self, p, ch, g, R):
        """set_gain_ramp(R) then set_output_gain(ch, g)"""
        self._ev(p, "gain", ch, g, R)

    def reset_overflow(self, p):
        self._ev(p, "reset")

    def update(self, f, s, h):
        """update_coeff of an idle set: later commits onto set s use these taps"""
        self.h[f].append(np.asarray(h, np.float64))
        self.hd[f].append(_digest(self.h[f][-1]))
        self.sets[f][s] = len(self.h[f]) - 1

    def commit(self, p, mode, F, changes):
        """the request group {f: (set or None, gain or None)} committed by block call p"""
        new = list(self.asg)
        for f, (s, g) in changes.items():
            new[f] = (new[f][0] if s is None else self.sets[f][s], new[f][1] if g is None else g)
        assert new != self.asg
        self.asg = new
        self.commits.append((p * self.L0, mode, F, new))

    # ---- the expected output
    def _side(self, io, raw, periods):
        """mute and delay lines of one side over the raw stream [periods * L0 * frame bytes]"""
        nb = self.fmts[io][0].bytes
        n_ch = (self.n_in, self.n_out)[io]
        # a channel without a filter on a side that uses sub-delay: sdf_length whole frames more in its
        # line (added to the delay and to a non-negative maxdelay)
        extra = [self.half if (self.half and self.sub0[io] and ch not in self.sub0[io]) else 0 for ch in range(n_ch)]
        lines = []
        for ch in range(n_ch):
            init, maxd = self.delay[io].get(ch, (0, -1))
            lines.append(Line(io, init + extra[ch], maxd + extra[ch] if maxd >= 0 else maxd, nb, self.L0))
        fb = n_ch * nb
        out = np.ascontiguousarray(raw, np.uint8).reshape(periods, self.L0, fb).copy()
        for p in range(periods):
            for kind, a in self.events.get(p, ()):
                if kind == "delay" and a[0] == io:
                    lines[a[1]].req = a[2] + extra[a[1]]
                if kind == "mute" and a[0] == io:
                    lines[a[1]].muted = a[2]
            for ch, ln in enumerate(lines):
                if ln.d or ln.muted:
                    ln.run(out[p], ch)
        self.cur_delay[io] = [ln.cur - e for ln, e in zip(lines, extra)]
        return out.ravel()

    def _vals(self, io, ch, periods):
        v, out = self.sub0[io][ch], []
        for p in range(periods):
            for kind, a in self.events.get(p, ()):
                if kind == "sub" and a[:2] == (io, ch):
                    v = a[2]
            out.append(v)
        return out

    def inputs(self, x_raw, periods):
        """the reals the segments read: [frames][n_in]"""
        n = periods * self.L0
        xr = nr.decode(self._side(IN, x_raw, periods), self.fmts[IN], n)
        for ch in self.sub0[IN]:
            xr[:, ch] = fir(xr[:, ch], self._vals(IN, ch, periods), self.half, self.rs, self.L0)
        return xr

    def yseg(self, x, asg):
        """[segment][frames][n_out] under the assignment.  A filter's segment outputs are kept under
        what they are a function of -- the schedule, the input channel's samples and the taps -- so
        a cache shared between Chains can only ever return the right array."""
        out = np.zeros((len(self.sched[0]), len(x), self.n_out))
        sk = (tuple(self.sched[0]), tuple(self.sched[1]))
        xd = [_digest(x[:, i]) for i in range(self.n_in)]
        for f, (v, gain) in enumerate(asg):
            i, o, si, so = self.filters[f]
            key = (sk, xd[i], self.hd[f][v])
            if key not in self._y:
                self._y[key] = sr.segment_outputs(x, [(i, 0, self.h[f][v], 1.0)], self.sched, 1)[:, :, 0]
            out[:, :, o] += self._y[key] * (si * so * gain)
        return out

    def gains(self, periods):
        gr = GainRamp(periods * self.L0, self.L0, [1.0] * self.n_out)
        for p in range(periods):
            for kind, a in self.events.get(p, ()):
                if kind == "gain":
                    gr.set_ramp(a[2])
                    gr.request(a[0], a[1])
            gr.commit(p)
        return gr.g

    def render(self, x_raw, periods, frames=None):
        n, L0 = periods * self.L0, self.L0
        x = self.inputs(x_raw, periods)
        start = [(0, 1.0)] * len(self.filters)
        ys = [self.yseg(x, start)] + [self.yseg(x, a) for _, _, _, a in self.commits]
        y = blend(ys, [(t, m, F, k + 1) for k, (t, m, F, _) in enumerate(self.commits)], self.sched, frames)
        y = y * self.gains(periods)
        if self.sub0[OUT]:
            scale = np.array([f.scale for f in self.fmts[OUT]])
            y = y / scale
            for ch in self.sub0[OUT]:
                y[:, ch] = fir(y[:, ch], self._vals(OUT, ch, periods), self.half, self.rs, L0)
            y = y * scale
        resets = [p for p in range(periods) if any(k == "reset" for k, _ in self.events.get(p, ()))]
        raw, of, status = nr.encode(y, self.fmts[OUT], L0, dither=self.dither, rate=self.rate, resets=resets)
        return Result(self._side(OUT, raw, periods), of, status, y)


# ---------------------------------------------------------------- sessions

SMALL = sr.SMALL
SESSION_SCHEDS = (SMALL, ([512, 1024], [2, 2]), ([64, 16384], [255, 2]))
KINDS = ("commit", "update", "gain", "delay", "mute", "subdelay", "reset")
SESSION_BASE = 7004      # seeds 0-7 on it draw every schedule, both switch modes per precision and a dithered output


def session(seed):
    """the setup and the event list of one session, a pure function of the seed.  A 2x2 crossbar with
    two sets per filter.  Input 0 and output 1 have a sub-delay filter, input 1 and both outputs a
    changeable delay line.  Events: (period, kind, args), sorted by period, each in front of that
    period's block call:
        commit    (mode, F, {f: (set or None, gain or None)})   set_coeff / set_filter_gain group
        update    (f, set, seed of the new taps)                 update_coeff of an idle set
        gain      (ch, g, R)                                     set_gain_ramp(R), set_output_gain
        delay     (io, ch, d)     mute (io, ch, m)     subdelay (io, ch, v)     reset ()
    Consecutive commits are at least taps + F + 2 L_max frames apart."""
    rng = np.random.default_rng(SESSION_BASE + seed)
    rs = 4 if seed % 2 == 0 else 8
    sched = SESSION_SCHEDS[int(rng.integers(3))]
    L0, Lmax = sched[0][0], sched[0][-1]
    taps_n = sum(L * N for L, N in zip(*sched))
    if rs == 4:                                   # float32 resolves a count at 16 bits only
        infmt = str(rng.choice(["S16_LE", "S24_LE", "FLOAT_LE"]))
        outfmt = str(rng.choice(["S16_LE", "FLOAT_LE"]))
        dither = ()
    else:
        infmt = str(rng.choice(["S16_LE", "S24_4LE", "S32_LE", "FLOAT64_LE"]))
        outfmt = str(rng.choice(["S16_LE", "S24_LE", "S32_LE", "FLOAT64_LE"]))
        # Dither on 16- and 24-bit outputs only.  The HP-TPDF chain feeds its error back as
        # v[n] = x[n] + s[n-1] - s[n-2], s[n] = v[n] - out[n]: poles on the unit circle, so the rounding
        # difference between device and model (about 1e-15 of the signal, in counts) does not die out in
        # the feedback state but walks, and the expected number of samples that round the other way
        # grows with frames^1.5 / (size of a count).  _close's 12 samples were set on 9000-frame S16 runs;
        # a 250 000-frame session meets them with room at 16 and 24 bits (expected << 1 tie), at 32 bits
        # (a count is 4.7e-10 of full scale) it was measured AT the limit: 4 ties, 12 samples.
        dither = [(0,), (1,), (0, 1)][int(rng.integers(3))] if outfmt in ("S16_LE", "S24_LE") else ()
    half = int(rng.choice([7, 15, 31]))
    ev, p = [], int(rng.integers(3, 9))
    for k in range(3):
        mode = int(rng.integers(2)) if k else seed // 2 % 2
        F = int(rng.choice([0, 2, L0, 700, 5 * L0 + 3]))
        if k == 0:
            ch = {f: (1, None) for f in range(4)}
            ch[int(rng.integers(4))] = (1, float(rng.choice([-1.0, 0.5, 2.0])))
        elif k == 1:
            # set 0 is idle since the first commit: rewritten one to three periods back (the stretch
            # between commits has three periods to spare for that), now switched onto
            f_up = int(rng.integers(4))
            ev.append((p - int(rng.integers(1, 4)), "update", (f_up, 0, 9000 + seed)))
            ch = {f_up: (0, None), (f_up + 1) % 4: (None, float(rng.choice([0.0, -0.5, 1.5])))}
        else:
            ch = {int(rng.integers(4)): (None, 0.75)}                     # gain only
        ev.append((p, "commit", (mode, F, ch)))
        gap = -(-(taps_n + F + 2 * Lmax) // L0)
        q = p + gap + 3 + int(rng.integers(0, 6))
        # the other controls, spread over the stretch up to the next commit (or the end)
        span = q - p
        at = lambda lo, hi: p + int(rng.integers(max(1, int(lo * span)), max(1, int(lo * span)) + max(1, int((hi - lo) * span))))
        if k == 0:
            ev.append((at(0.0, 0.1), "gain", (0, 30.0, int(rng.choice([0, 48, 150, 3 * L0 + 5])))))   # clips integers
            ev.append((at(0.3, 0.4), "gain", (0, 1.0, int(rng.choice([1, 64, 700])))))
            ev.append((at(0.6, 0.7), "reset", ()))
            ev.append((at(0.1, 0.5), "mute", (IN, 0, 1)))
            ev.append((at(0.5, 0.9), "mute", (IN, 0, 0)))
        elif k == 1:
            ev.append((at(0.0, 0.05), "gain", (1, float(rng.choice([0.0, 0.3, 2.5])), int(rng.choice([0, 100, 2 * L0])))))
            ev.append((at(0.1, 0.3), "mute", (OUT, 1, 1)))
            ev.append((at(0.3, 0.5), "mute", (OUT, 1, 0)))
            ev.append((at(0.5, 0.9), "gain", (1, 1.0, 900)))
        else:
            ev.append((at(0.1, 0.2), "gain", (0, 30.0, int(rng.choice([0, 100])))))                   # clips behind the reset
            ev.append((at(0.5, 0.6), "gain", (0, 1.0, 64)))
        for io, chn in ((IN, 1), (OUT, 0), (OUT, 1)):
            for lo in (0.05, 0.55):
                d = int(rng.choice([0, 1, L0 - 1, L0, L0 + 1, 2 * L0 + 5, 3 * L0]))      # 3 L0: above OUT's maxdelay
                ev.append((at(lo, lo + 0.4), "delay", (io, chn, d)))
        for io, chn in ((IN, 0), (OUT, 1)):
            ev.append((at(0.0, 0.9), "subdelay", (io, chn, int(rng.choice([-99, -37, 0, 12, 50, 99])))))
        p = q
    ev.sort(key=lambda e: e[0])                   # stable: calls of one period keep their order
    return dict(seed=seed, rs=rs, sched=sched, infmt=infmt, outfmt=outfmt, dither=tuple(dither), half=half,
                maxdelay={(IN, 1): 3 * L0, (OUT, 0): 2 * L0 + 5, (OUT, 1): 2 * L0 + 5},
                periods=p, events=ev)
