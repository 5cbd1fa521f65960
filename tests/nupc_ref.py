"""Float64 reference model of the non-uniform partitioned convolver (include/bfhip_nupc.h), for
the tests.  It knows nothing about segments: the convolver's output is defined as the plain
linear convolution of the decoded inputs, requantised period by period, so the model is

    decode   raw -> reals with the oracle's Ctx.raw2real (the reference's raw2real) times the
             input format's scale,
    convolve per output, in float64 (numpy FFT): the sum over its filters of
             in_scale * out_scale * (x_in * taps), cut to the frames run,
    blend    a coefficient switch at frame t_sw with an F-frame cross-fade (the header's
             definition: old before t_sw, (1 - w) old + w new with w = (t - t_sw) / (F - 1) in
             [t_sw, t_sw + F), new afterwards; F = 0 is a hard switch),
    encode   times the output gain, divided by the output format's scale, through the oracle's
             Ctx.cbuf2raw (the reference's real2raw, HP-TPDF dither included) one L0-frame period
             at a time: the expected raw bytes and overflow counters.

Nothing here touches a device or the reference tree: numpy and the oracle library only."""
import numpy as np

import bforacle as bo


def fmt(name, spacing=1, offset=0):
    return bo.make_format(name, spacing, offset)


def layout(names, gap=0, order=None):
    """formats of one side, one frame: channel c in slot order[c] of a frame of len(names) + gap
    samples (the gap samples are bytes nobody owns).  All names must have one byte width."""
    width = {bo.SAMPLE_FORMATS[n][0] for n in names}
    assert len(width) == 1, names
    nb = width.pop()
    order = list(range(len(names))) if order is None else list(order)
    spacing = len(names) + gap
    return [fmt(n, spacing, order[c] * nb) for c, n in enumerate(names)]


def frame_bytes(fmts):
    return fmts[0].sample_spacing * fmts[0].bytes


def pack(x, fmts, fill=0xA5):
    """reals in raw units ([frames][channels]; integers for integer formats) -> the raw stream.
    Gap bytes hold `fill` so that a reader of the wrong bytes sees garbage, not silence."""
    n = len(x)
    buf = np.full(n * frame_bytes(fmts), fill, np.uint8)
    for c, f in enumerate(fmts):
        nb, sb = f.bytes, f.sbytes
        if f.isfloat:
            raw = np.ascontiguousarray(x[:, c].astype(np.float32 if nb == 4 else np.float64)).view(np.uint8).reshape(n, nb)
        else:
            q = np.asarray(x[:, c], np.int64)
            assert q.min() >= -(1 << (8 * sb - 1)) and q.max() < (1 << (8 * sb - 1))
            raw = np.stack([(q >> (8 * k)) & 0xff for k in range(nb)], axis=1).astype(np.uint8)
        if f.swap:
            raw = raw[:, ::-1]
        idx = f.byte_offset + np.arange(n)[:, None] * frame_bytes(fmts) + np.arange(nb)[None, :]
        buf[idx] = raw
    return buf


def decode(raw, fmts, n_frames, scaled=True):
    """raw stream -> float64 [frames][channels] with the oracle's raw2real (the reference's), times
    the format's scale unless scaled=False (then integer formats give their integers)"""
    ctx = bo.Ctx(4, 8)
    raw = np.ascontiguousarray(raw, np.uint8)
    out = np.zeros((n_frames, len(fmts)))
    for c, f in enumerate(fmts):
        v = ctx.raw2real(raw[f.byte_offset:], f.bytes, f.isfloat, f.sample_spacing, f.swap, n_frames)
        out[:, c] = v * (f.scale if scaled else 1.0)
    return out


def conv(x, h, n):
    """float64 linear convolution of x with h, first n frames"""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    m = min(len(x), n) + len(h) - 1
    nfft = 1 << max(m - 1, 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x[:n], nfft) * np.fft.rfft(h, nfft), nfft)[:n]


def convolve(x, filters, n_out):
    """x: [frames][n_in] decoded, scaled inputs; filters: (in, out, taps, in_scale, out_scale)
    -> [frames][n_out] float64, the sum over each output's filters"""
    n = len(x)
    y = np.zeros((n, n_out))
    for i, o, h, si, so in filters:
        y[:, o] += conv(x[:, i], h, n) * (si * so)
    return y


def crossfade(y_old, y_new, t_sw, F):
    """the output of a switch from y_old to y_new at frame t_sw with an F-frame fade"""
    out = y_old.copy()
    n = len(out)
    if t_sw >= n:
        return out
    out[t_sw:] = y_new[t_sw:]
    if F:
        j = np.arange(min(F, n - t_sw))
        w = (j / (F - 1.0)).reshape((-1,) + (1,) * (out.ndim - 1))
        out[t_sw:t_sw + len(j)] = (1 - w) * y_old[t_sw:t_sw + len(j)] + w * y_new[t_sw:t_sw + len(j)]
    return out


def switched(ys, switches):
    """ys[k]: output under assignment k; switches: [(t_sw, F, k)] in order, starting from
    assignment 0 -> the blended output"""
    out = ys[0].copy()
    for t, F, k in switches:
        out = crossfade(out, ys[k], t, F)
    return out


def new_overflows(fmts, start=None):
    """the library's initial overflow structs (max = full scale - 1 for integers, 1.0 for floats),
    or copies of `start`"""
    if start is not None:
        return [bo.Overflow(*s.astuple()) for s in start]
    return [bo.Overflow(0, 0, 0.0, 1.0 if f.isfloat else float((1 << (8 * f.sbytes - 1)) - 1)) for f in fmts]


def encode(y, fmts, L0, gain=None, dither=(), rate=44100, max_size=0, overflow=None, safety_limit=0.0, resets=()):
    """y: [frames][n_out] float64 reals; gain: per-channel factors, or [frames][n_out]; dither:
    ascending output channels with HP-TPDF dither (slot = rank); resets: periods in front of which
    the overflow structs go back to their initial value (the dither walk goes on).  Returns (raw
    stream, overflow structs, status bits per period).  Periods of L0 frames, as the library
    quantises them."""
    n, n_out = y.shape
    assert n % L0 == 0
    g = np.ones(n_out) if gain is None else np.asarray(gain, np.float64)
    v = y * g / np.array([f.scale for f in fmts])
    ctx = bo.Ctx(L0, 8)
    if dither:
        assert ctx.dither_init(len(dither), rate, max_size)
    fb = frame_bytes(fmts)
    of = new_overflows(fmts, overflow)
    raw = np.zeros(n * fb, np.uint8)
    status = []
    for b in range(n // L0):
        st_all = 0
        if b in resets:
            of = new_overflows(fmts)
        for c, f in enumerate(fmts):
            d = list(dither).index(c) if c in dither else -1
            seg = np.ascontiguousarray(v[b * L0:(b + 1) * L0, c])
            st, r = ctx.cbuf2raw(seg, f, L0 * fb, of[c], dither_channel=d, safety_limit=safety_limit)
            st_all |= st
            idx = f.byte_offset + np.arange(L0)[:, None] * fb + np.arange(f.bytes)[None, :]
            raw[b * L0 * fb + idx] = r[idx]
        status.append(st_all)
    return raw, of, status


def ints(raw, fmts, n_frames):
    """the integer samples of integer-format channels (float channels: their values)"""
    return decode(raw, fmts, n_frames, scaled=False)
