"""Float64 reference model of the crossbar engine's block semantics (include/bfhip.h), for the
tests.  It knows nothing about partitions, rings or plans, and uses neither the oracle nor the
engine: numpy and scipy only.

    decode   raw interleaved blocks -> float64, exactly (integers times 2^-(bits-1), floats as
             they are);
    inputs   a virtual input of an N:1 input map is its physical channel delayed by its sample
             delay, and zero from the block it is muted at;
    filters  each filter (input, output) has a per-block timeline of states: the taps in force,
             delayblocks (clamped to N - 1, the taps then cut to N - d partitions: cblocks_of,
             bfrun.c:1579-1591), the input and output scales, and whether the block of a change is
             a cross-fade;
    output   block t is the sum over filters of block t of scale * conv(x delayed by d_t * B, h_t)
             while the delay and input scale have been constant for N blocks; after a run-time
             change the filter's ring is followed slot by slot (output()); on a cross-fade block the ramp (1 - w) old + w new, w = k / (B - 1)
             (cases.fade_cascade_network, fftw_convolver.c:330-368);
    encode   integer formats requantised in float64 the way the reference's no-dither real2raw
             does (+0.5, truncate, clip), with its overflow records and status bits.

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


class Filter:
    """one filter of the crossbar: input channel, output channel and its timeline of states"""

    def __init__(self, i, o, taps, delay=0, in_scale=1.0, out_scale=1.0):
        self.i, self.o = i, o
        self.segs = [(0, dict(taps=np.asarray(taps, np.float64), delay=delay, in_scale=in_scale,
                              out_scale=out_scale), False)]

    @property
    def state(self):
        return self.segs[-1][1]

    def change(self, t, fade=False, **kw):
        """from block t on: the state with `kw` changed; fade: block t is a cross-fade from the state
        before (several changes at one block merge; the fade flag is kept if any asked for it)"""
        st = dict(self.state)
        st.update(kw)
        if "taps" in kw:
            st["taps"] = np.asarray(kw["taps"], np.float64)
        if self.segs[-1][0] == t and t > 0:
            _, _, f0 = self.segs.pop()
            fade = fade or f0
        assert not self.segs or t >= self.segs[-1][0]
        self.segs.append((t, st, fade))


def _window_out(x, s, h_i, L):
    """the B outputs one ring slot adds: window [x_(s-1) | x_s] of block s through partition h_i"""
    w = np.zeros(2 * L)
    if s >= 1:
        w[:L] = x[(s - 1) * L:s * L]
    w[L:] = x[s * L:(s + 1) * L]
    return fftconvolve(w, h_i)[L:2 * L]


def output(x, filters, L, N, n_out, n_blocks):
    """x: [frames][n_in] float64 inputs (virtual ones for an input map); -> [n_blocks * L][n_out].

    Delays and input scales act where the reference applies them: when a block ENTERS the
    filter's ring (block s goes to slot (s + d_s) mod N scaled by a_s, bfrun.c:1600-1641; output
    block t reads slots t - i, i < min(cblocks, blocks processed)).  While every block in the ring
    entered with the delay and scale in force, that is scale * conv(x delayed by d B, h cut to
    N - d partitions): one fftconvolve per distinct state.  The N blocks after a run-time delay or
    input-scale change are summed slot by slot."""
    n = n_blocks * L
    y = np.zeros((n, n_out))
    w = np.arange(L) / (L - 1.0)
    clamp = lambda d: min(max(int(d), 0), N - 1)
    for f in filters:
        xi = x[:, f.i]
        starts = [s[0] for s in f.segs]
        st_of = [f.segs[int(np.searchsorted(starts, t, side="right")) - 1][1] for t in range(n_blocks)]
        entry = [(clamp(st["delay"]), st["in_scale"]) for st in st_of]
        cache = {}

        def full(st):
            d = clamp(st["delay"])
            key = (id(st["taps"]), d, st["in_scale"])
            if key not in cache:
                h = st["taps"][:(N - d) * L]
                xd = np.zeros(n)
                xd[d * L:] = xi[:n - d * L]
                cache[key] = fftconvolve(xd, h)[:n] * st["in_scale"] if len(h) else np.zeros(n)
            return cache[key]

        def block(t, st):
            d, a = clamp(st["delay"]), st["in_scale"]
            if all(entry[s] == (d, a) for s in range(max(0, t - N + 1), t + 1)):
                return full(st)[t * L:(t + 1) * L] * st["out_scale"]
            h = st["taps"][:(N - d) * L]
            cb = (len(h) + L - 1) // L
            out = np.zeros(L)
            for i in range(min(cb, t + 1, N)):
                j = (t - i) % N
                writers = [s for s in range(t + 1) if (s + entry[s][0]) % N == j]
                if not writers:
                    continue
                s = writers[-1]
                out += entry[s][1] * _window_out(xi, s, h[i * L:(i + 1) * L], L)
            return out * st["out_scale"]

        for t in range(n_blocks):
            k = int(np.searchsorted(starts, t, side="right")) - 1
            t0, st, fade = f.segs[k]
            r = block(t, st)
            if fade and t == t0 and k > 0:
                r = (1 - w) * block(t, f.segs[k - 1][1]) + w * r
            y[t * L:(t + 1) * L, f.o] += r
    return y
