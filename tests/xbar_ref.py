"""Float64 reference model of the crossbar engine's block semantics (include/bfhip.h), for the
tests.  It knows nothing about partitions, rings or plans, and uses neither the oracle nor the
engine: numpy and scipy only.  (The Channels layer at the end is the exception: it borrows the
FFT-free codecs of nupc_ref -- the oracle's raw2real / real2raw -- and is handed its sub-sample
filters by the caller.)

    decode   raw interleaved blocks -> float64, exactly (integers times 2^-(bits-1), floats as
             they are);
    inputs   a virtual input of an N:1 input map is its physical channel delayed by its sample
             delay, and zero from the block it is muted at;
    filters  each filter (channel inputs, filter inputs, outputs) has a per-block timeline of
             states: the taps in force (a dirac: DIRAC; a short or scaled set: coeff()),
             delayblocks (clamped to N - 1, the taps then cut to N - d partitions: cblocks_of,
             bfrun.c:1579-1591), the input, filter-input and output scales, and whether the block
             of a change is a cross-fade; filters are evaluated in list order, a filter input
             reading an earlier filter's unscaled output;
    output   block t is the sum over filters of block t of scale * conv(x delayed by d_t * B, h_t)
             while the delay and input scale have been constant for N blocks; after a run-time
             change the filter's ring is followed slot by slot (output()); on a cross-fade block the ramp (1 - w) old + w new, w = k / (B - 1)
             (cases.fade_cascade_network, fftw_convolver.c:330-368);
    encode   integer formats requantised in float64 the way the reference's no-dither real2raw
             does (+0.5, truncate, clip), with its overflow records and status bits.

    channels the stage between the raw buffers and the network (Channels): formats, N:1 maps with
             integer delay and mute, the sub-sample delay FIR, the mix of a shared output, one
             quantisation (HP-TPDF dither included) per physical output.

One fftconvolve per distinct filter state, not per block, so that the model stays
cheap at L = 8192."""
import numpy as np
from scipy.signal import fftconvolve

# name: (bytes, significant bytes, float)
FORMATS = {"S16_LE": (2, 2, False), "S24_LE": (3, 3, False), "S24_4LE": (4, 3, False),
           "S32_LE": (4, 4, False), "FLOAT_LE": (4, 4, True), "FLOAT64_LE": (8, 8, True)}
ST_NONFINITE, ST_SAFETY = 1, 2


def decode(raw, name, n_ch):
    """raw interleaved frames (bytes, or an array of the sample type) -> float64 [frames][n_ch]"""
    nb, sb, isfloat = FORMATS[name]
    b = np.ascontiguousarray(raw).view(np.uint8).ravel()
    n = len(b) // (nb * n_ch)
    b = b[:n * nb * n_ch].reshape(n, n_ch, nb)
    if isfloat:
        return b.copy().view(np.float32 if nb == 4 else np.float64)[..., 0].astype(np.float64)
    v = np.zeros((n, n_ch), np.int64)
    for k in range(sb):                               # the low sb bytes, little-endian
        v |= b[..., k].astype(np.int64) << (8 * k)
    v = np.where(v >= 1 << (8 * sb - 1), v - (1 << (8 * sb)), v)
    return v.astype(np.float64) / float(1 << (8 * sb - 1))


class Overflow:
    """struct bfoverflow: n_overflows, intlargest, largest, max (raw units)"""

    def __init__(self, name):
        nb, sb, isfloat = FORMATS[name]
        self.n_overflows, self.intlargest, self.largest = 0, 0, 0.0
        self.max = 1.0 if isfloat else float((1 << (8 * sb - 1)) - 1)

    def astuple(self):
        return (self.n_overflows, self.intlargest, self.largest, self.max)


def quantise(v, name, of):
    """one block of one channel, v in raw units -> (integer samples, or float32 / float64 values),
    with `of` updated (real2raw without dither: v + 0.5, truncated toward zero, one less below zero,
    clipped at the format's limits; overflow counted and `largest` taken on the clipped ones only)"""
    nb, sb, isfloat = FORMATS[name]
    if isfloat:
        a = np.abs(v)
        of.n_overflows += int((a > of.max).sum())
        of.largest = max(of.largest, float(a.max(initial=0.0)))
        return v.astype(np.float32 if nb == 4 else np.float64)
    imin, imax = -(1 << (8 * sb - 1)), (1 << (8 * sb - 1)) - 1
    u = v + 0.5
    s = np.trunc(u)
    s = np.where(u < 0, s - 1, s)
    lo, hi = u <= imin, u > imax
    clip = lo | hi
    of.n_overflows += int(clip.sum())
    if clip.any():
        of.largest = max(of.largest, float(np.abs(u[clip]).max()))
    s = np.where(lo, imin, np.where(hi, imax, s)).astype(np.int64)
    if (~clip).any():
        of.intlargest = max(of.intlargest, int(np.abs(s[~clip]).max()))
    return s


def threshold_distance(v):
    """how close (in LSB) any sample in raw units comes to a rounding threshold of the quantiser
    (v + 0.5 an integer): where float32 rounding could flip the result"""
    u = np.asarray(v, np.float64) + 0.5
    return float(np.abs(u - np.round(u)).min(initial=1.0))


def encode(y, name, L, overflow=None, safety_limit=0.0):
    """y: [frames][channels] float64 reals (unit scale).  Returns (samples [frames][channels] in
    raw units: ints or floats, overflow structs, status bits per block).  A block whose status is
    not 0 stops the channel's conversion there, as real2raw does; its samples are not defined."""
    nb, sb, isfloat = FORMATS[name]
    n, n_ch = y.shape
    v = y * (1.0 if isfloat else float(1 << (8 * sb - 1)))
    ofs = [Overflow(name) for _ in range(n_ch)] if overflow is None else overflow
    out = np.zeros((n, n_ch), np.float64 if isfloat else np.int64)
    status = []
    for b in range(n // L):
        st = 0
        for c in range(n_ch):
            seg = v[b * L:(b + 1) * L, c]
            if not np.isfinite(seg).all():
                st |= ST_NONFINITE
                continue
            if safety_limit and (np.abs(seg) > safety_limit * ofs[c].max).any():
                st |= ST_SAFETY
                continue
            out[b * L:(b + 1) * L, c] = quantise(seg, name, ofs[c])
        status.append(st)
    return out, ofs, status


def virtual_inputs(x, virt2phys, delay=None, mute_from=None, L=None):
    """x: [frames][n_phys] decoded physical inputs -> [frames][n_virt]: virtual v is channel
    virt2phys[v] delayed by delay[v] samples, zero from block mute_from[v] on"""
    n = len(x)
    out = np.zeros((n, len(virt2phys)))
    for v, p in enumerate(virt2phys):
        d = (delay or {}).get(v, 0)
        out[d:, v] = x[:n - d, p]
        m = (mute_from or {}).get(v)
        if m is not None:
            out[m * L:, v] = 0.0
    return out


DIRAC = None       # the taps of a dirac filter (coeff = -1): the input, delayed by the filter's delay


def coeff(taps, L, scale=1.0, n_blocks=0):
    """the taps a coefficient set holds (add_coeff): scale * taps, cut to n_blocks partitions when
    n_blocks is given (a short set), as coeffs2cbuf renders them"""
    taps = np.asarray(taps, np.float64)
    if n_blocks > 0:
        taps = taps[:n_blocks * L]
    return taps * scale


def _vec(v, n):
    if v is None:
        return (1.0,) * n
    if np.isscalar(v):
        return (float(v),) * n
    v = tuple(float(a) for a in v)
    assert len(v) == n, (v, n)
    return v


def _taps(t):
    return np.ones(1) if t is None else np.asarray(t, np.float64)


class Filter:
    """one filter: channel inputs `i` (an index or a list) with their scales, filter inputs `in_f`
    (indices of earlier filters in the list handed to output()) with their scales, outputs `o` (an
    index or a list) with their scales, and its timeline of states"""

    def __init__(self, i, o, taps, delay=0, in_scale=1.0, out_scale=1.0, in_f=(), in_fscale=None):
        self.ins = [i] if np.isscalar(i) else list(i)
        self.outs = [o] if np.isscalar(o) else list(o)
        self.in_f = list(in_f)
        self.i, self.o = i, o
        self.segs = [(0, dict(taps=_taps(taps), delay=delay, in_scale=_vec(in_scale, len(self.ins)),
                              out_scale=_vec(out_scale, len(self.outs)),
                              fscale=_vec(in_fscale, len(self.in_f))), False)]

    @property
    def state(self):
        return self.segs[-1][1]

    def change(self, t, fade=False, **kw):
        """from block t on: the state with `kw` changed; fade: block t is a cross-fade from the taps
        before (several changes at one block merge; the fade flag is kept if any asked for it)"""
        st = dict(self.state)
        n = {"in_scale": len(self.ins), "out_scale": len(self.outs), "fscale": len(self.in_f)}
        for k, v in kw.items():
            st[k] = _taps(v) if k == "taps" else _vec(v, n[k]) if k in n else v
        if self.segs[-1][0] == t and t > 0:
            _, _, f0 = self.segs.pop()
            fade = fade or f0
        assert not self.segs or t >= self.segs[-1][0]
        self.segs.append((t, st, fade))

    def set_scale(self, t, io, idx, v):
        """set_scale(filter, io, idx, v) issued before block t"""
        key = "in_scale" if io == 0 else "out_scale"
        s = list(self.state[key])
        s[idx] = v
        self.change(t, **{key: s})

    def set_fscale(self, t, idx, v):
        s = list(self.state["fscale"])
        s[idx] = v
        self.change(t, fscale=s)


def _window_out(w, h_i, L):
    """the L outputs one ring slot adds: the 2L window w through partition h_i"""
    return fftconvolve(w, h_i)[L:2 * L]


def output(x, filters, L, N, n_out, n_blocks):
    """x: [frames][n_in] float64 inputs (virtual ones for an input map); -> [n_blocks * L][n_out].

    What enters a filter's ring at block s is the 2L window of its mixed input, sum_k a_s[k] x_k over
    blocks s-1 and s, plus, for filter inputs, sum_j fs[j] u_j (u_j: the unscaled time output of
    upstream filter j, its cross-fade ramp included) with the fscale in force at block s-1 in the
    first half and at block s in the second (convolve_eval keeps the mixed half of the last block,
    fftw_convolver.c:411-433).  Delays and input scales act where the reference applies them: when a
    block ENTERS the filter's ring (block s goes to slot (s + d_s) mod N scaled by a_s,
    bfrun.c:1600-1641; output block t reads slots t - i, i < min(cblocks, blocks processed)).  While
    every block in the ring entered with the delay and scales in force, that is conv(mixed input
    delayed by d B, h cut to N - d partitions): one fftconvolve per distinct state.  The N blocks
    after a run-time delay, input-scale or fscale change are summed slot by slot.  A cross-fade
    block is (1 - w) old + w new, w = k / (B - 1), the old taps read through the same ring
    (bfrun.c:1725-1777); output scales act on the block they are set for."""
    n = n_blocks * L
    y = np.zeros((n, n_out))
    z = []                                            # per filter: unscaled time output
    w = np.arange(L) / (L - 1.0)
    clamp = lambda d: min(max(int(d), 0), N - 1)      # noqa: E731
    for fi, f in enumerate(filters):
        assert all(0 <= j < fi for j in f.in_f), "filter inputs must precede"
        starts = [s[0] for s in f.segs]
        st_of = [f.segs[int(np.searchsorted(starts, t, side="right")) - 1][1] for t in range(n_blocks)]
        entry = [(clamp(st["delay"]), st["in_scale"], st["fscale"]) for st in st_of]
        cache, parts = {}, {}

        def part(kind, v):
            """sum_k a[k] x_k ("a") or sum_j fs[j] u_j ("fs") over the whole run"""
            if (kind, v) not in parts:
                m = np.zeros(n)
                for k, c in enumerate(f.ins if kind == "a" else f.in_f):
                    m += v[k] * (x[:n, c] if kind == "a" else z[c])
                parts[(kind, v)] = m
            return parts[(kind, v)]

        def mixed(a, fs):
            return part("a", a) + part("fs", fs) if f.in_f else part("a", a)

        def window(s):
            """the 2L window block s put in the ring"""
            _, a, fs = entry[s]
            w2 = np.zeros(2 * L)
            w2[L:] = part("a", a)[s * L:(s + 1) * L]
            if f.in_f:
                w2[L:] += part("fs", fs)[s * L:(s + 1) * L]
            if s >= 1:
                w2[:L] = part("a", a)[(s - 1) * L:s * L]
                if f.in_f:
                    w2[:L] += part("fs", entry[s - 1][2])[(s - 1) * L:s * L]
            return w2

        def full(st):
            d = clamp(st["delay"])
            key = (id(st["taps"]), d, st["in_scale"], st["fscale"])
            if key not in cache:
                h = st["taps"][:(N - d) * L]
                xd = np.zeros(n)
                xd[d * L:] = mixed(st["in_scale"], st["fscale"])[:n - d * L]
                cache[key] = fftconvolve(xd, h)[:n] if len(h) else np.zeros(n)
            return cache[key]

        def block(t, st):
            d = clamp(st["delay"])
            key = (d, st["in_scale"], st["fscale"])
            if all(entry[s] == key for s in range(max(0, t - N + 1), t + 1)) and \
                    (t < N or entry[t - N][2] == st["fscale"]):
                return full(st)[t * L:(t + 1) * L]
            h = st["taps"][:(N - d) * L]
            cb = (len(h) + L - 1) // L
            out = np.zeros(L)
            for i in range(min(cb, t + 1, N)):
                j = (t - i) % N
                writers = [s for s in range(t + 1) if (s + entry[s][0]) % N == j]
                if writers:
                    out += _window_out(window(writers[-1]), h[i * L:(i + 1) * L], L)
            return out

        zf = np.zeros(n)
        for t in range(n_blocks):
            k = int(np.searchsorted(starts, t, side="right")) - 1
            t0, st, fade = f.segs[k]
            r = block(t, st)
            if fade and t == t0 and k > 0:
                r = (1 - w) * block(t, dict(st, taps=f.segs[k - 1][1]["taps"])) + w * r
            zf[t * L:(t + 1) * L] = r
            for c, g in zip(f.outs, st["out_scale"]):
                y[t * L:(t + 1) * L, c] += g * r
        z.append(zf)
    return y


# ------------------------------------------------------------------ networks (cases.build specs)

class Network:
    """the model of a filter network given as a cases.build spec (coeffs [(taps, scale, n_blocks)],
    filters [add_filter keywords]), and of the run-time calls made on it: act(t, a) for a call
    issued before block t, a one of ("coeff", f, c), ("scale", f, io, idx, v), ("fscale", f, idx,
    v), ("delay", f, d) -- the tuples cases.act() hands an engine"""

    def __init__(self, spec):
        self.spec, self.L, self.N = spec, spec["L"], spec["N"]
        self.cur = [fd.get("coeff", -1) for fd in spec["filters"]]
        self.filters = [Filter(fd.get("in_ch", ()), fd.get("out_ch", ()), self.taps(fd.get("coeff", -1)),
                               fd.get("delayblocks", 0),
                               fd.get("in_scale"), fd.get("out_scale"), fd.get("in_f", ()), fd.get("in_fscale"))
                        for fd in spec["filters"]]

    def taps(self, c):
        if c < 0:
            return DIRAC
        t, scale, nb = self.spec["coeffs"][c]
        return coeff(t, self.L, scale, nb)

    def act(self, t, a):
        f = self.filters[a[1]]
        if a[0] == "coeff":
            fade = bool(self.spec["filters"][a[1]].get("crossfade")) and a[2] != self.cur[a[1]]
            self.cur[a[1]] = a[2]
            f.change(t, fade=fade, taps=self.taps(a[2]))
        elif a[0] == "scale":
            f.set_scale(t, a[2], a[3], a[4])
        elif a[0] == "fscale":
            f.set_fscale(t, a[2], a[3])
        elif a[0] == "delay":
            f.change(t, delay=a[2])

    def output(self, x, n_blocks, actions=None):
        for t in sorted(actions or {}):
            for a in actions[t]:
                self.act(t, a)
        return output(x, self.filters, self.L, self.N, self.spec["n_out"], n_blocks)


# ------------------------------------------------------------------ the channel stage

def shifted(x, d):
    """the stream x delayed by d frames (zeros in front)"""
    out = np.zeros(len(x))
    if d < len(x):
        out[d:] = x[:len(x) - d]
    return out


def subdelay_fir(x, taps_per_block, L):
    """y[n] = sum_k h_t[k] x[n - k] over the continuous unfiltered stream x (x[n < 0] = 0), h_t the
    taps in force in block t = n // L (delay.c:416-442: the history is never the filtered signal)"""
    x = np.asarray(x, np.float64)
    y = np.zeros(len(x))
    for t, h in enumerate(taps_per_block):
        seg = np.concatenate([np.zeros(len(h) - 1), x])[t * L:(t + 1) * L + len(h) - 1]
        y[t * L:(t + 1) * L] = (fftconvolve(seg, h, mode="valid") if len(h) > 512 else
                                np.convolve(seg, h, mode="valid"))
    return y


class Channels:
    """The channel stage around a Network, in float64.  `ch` describes it:

        in_map / out_map   virt2phys per side (default: 1:1)
        in_fmt / out_fmt   sample format name of the side's physical channels (interleaved)
        delay, mute_from   {(io, v): frames} / {(io, v): block}: members of a shared channel only (a
                           1:1 channel's delay and mute are the sound-card layer's, dai.c)
        sdf_length         half length of the sub-sample filters, 0: none
        subdelay           {(io, v): value}: the channels that have a filter, and its first value
        dither             ascending physical outputs with HP-TPDF dither; rate, max_size

    taps_of(value) -> the 2 * sdf_length + 1 float64 taps of a sub-sample value.  Run-time changes:
    the Network's action tuples plus ("subdelay", io, v, value), issued before block t.

    Input side: virtual v is physical in_map[v]; a member of a shared input is delayed by delay[v],
    and by sdf_length more when the side filters any channel and v has no filter (bfrun.c:1152-1162,
    1512-1516), then zero from block mute_from[v] on; a filtered input then goes through its FIR.
    Output side (bfrun.c:1926-2003): the FIR; for members of a shared output the integer delay (+
    sdf_length as above) and the mute; the sum of the un-muted members in ascending order; one
    quantisation per physical output (nupc_ref.encode: the oracle's real2raw); every member of a
    shared output carries the group's overflow record."""

    def __init__(self, spec, ch, taps_of=None):
        self.spec, self.ch, self.taps_of = spec, ch, taps_of
        self.L, self.half = spec["L"], ch.get("sdf_length", 0)
        self.maps = [list(ch.get("in_map", range(spec["n_in"]))), list(ch.get("out_map", range(spec["n_out"])))]
        assert len(self.maps[0]) == spec["n_in"] and len(self.maps[1]) == spec["n_out"]
        self.sd = {k: [(0, v)] for k, v in ch.get("subdelay", {}).items()}     # (io, v): [(block, value)]
        self.net = Network(spec)

    def formats(self, io):
        import nupc_ref as nr
        n_phys = max(self.maps[io]) + 1
        return nr.layout([self.ch["in_fmt" if io == 0 else "out_fmt"]] * n_phys)

    def shared(self, io, v):
        return self.maps[io].count(self.maps[io][v]) > 1

    def _taps(self, io, v, n_blocks):
        seg = self.sd[(io, v)]
        starts = [s[0] for s in seg]
        return [self.taps_of(seg[int(np.searchsorted(starts, t, side="right")) - 1][1]) for t in range(n_blocks)]

    def _member(self, io, v, x):
        """delay and mute of virtual channel v (a member of a shared physical channel)"""
        filters = any(k[0] == io for k in self.sd)
        extra = self.half if filters and (io, v) not in self.sd else 0
        x = shifted(x, self.ch.get("delay", {}).get((io, v), 0) + extra)
        m = self.ch.get("mute_from", {}).get((io, v))
        if m is not None:
            x[m * self.L:] = 0.0
        return x

    def inputs(self, raw, n_blocks):
        """raw input stream -> [frames][n_in] float64 virtual inputs"""
        import nupc_ref as nr
        n = n_blocks * self.L
        x = nr.decode(np.ascontiguousarray(raw).view(np.uint8).ravel(), self.formats(0), n)
        out = np.zeros((n, len(self.maps[0])))
        for v, p in enumerate(self.maps[0]):
            s = self._member(0, v, x[:, p]) if self.shared(0, v) else x[:, p].copy()
            if (0, v) in self.sd:
                s = subdelay_fir(s, self._taps(0, v, n_blocks), self.L)
            out[:, v] = s
        return out

    def mix(self, y, n_blocks):
        """[frames][n_out] virtual outputs of the network -> [frames][n_phys] reals to quantise"""
        out = np.zeros((len(y), max(self.maps[1]) + 1))
        for v, p in enumerate(self.maps[1]):
            s = y[:, v]
            if (1, v) in self.sd:
                s = subdelay_fir(s, self._taps(1, v, n_blocks), self.L)
            if self.shared(1, v):
                s = self._member(1, v, s)
            out[:, p] += s
        return out

    def reals(self, raw, n_blocks, actions=None):
        """-> [frames][n_phys out] float64, unit scale: what the quantiser is handed"""
        net_actions = {}
        for t in sorted(actions or {}):
            for a in actions[t]:
                if a[0] == "subdelay":
                    assert (a[1], a[2]) in self.sd, "only a channel that starts with a filter has one"
                    self.sd[(a[1], a[2])].append((t, a[3]))
                else:
                    net_actions.setdefault(t, []).append(a)
        return self.mix(self.net.output(self.inputs(raw, n_blocks), n_blocks, net_actions), n_blocks)

    def run(self, raw, n_blocks, actions=None, safety_limit=0.0):
        """-> (y [frames][n_phys] reals, raw output stream, overflow records per VIRTUAL output,
        status per block)"""
        import nupc_ref as nr
        y = self.reals(raw, n_blocks, actions)
        out, ofs, status = nr.encode(y, self.formats(1), self.L, dither=tuple(self.ch.get("dither", ())),
                                     rate=self.ch.get("rate", 44100), max_size=self.ch.get("max_size", 0),
                                     safety_limit=safety_limit)
        return y, out, [ofs[p] for p in self.maps[1]], status
