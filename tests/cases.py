"""Shared builders: the same configuration is instantiated in the oracle (oracle/bforacle.py)
and in the HIP engine (brutefir_amd.Engine) -- both expose the same methods -- and driven with
the same seeded raw input blocks."""
import numpy as np

RAW_NP = {"S8": np.int8, "S16_LE": np.int16, "S32_LE": np.int32, "S24_4LE": np.int32,
          "FLOAT_LE": np.float32, "FLOAT64_LE": np.float64}


def make_ir(rng, taps, n_in):
    """white noise * exponential decay, normalised so that n_in summed filters stay inside
    +-1 (synthetic inputs)"""
    h = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.0))
    return h / (np.abs(h).sum() * n_in)


def crossbar(engine_cls, L, N, rs, I, O, infmt="S24_4LE", outfmt="S24_4LE", seed=4321,
             taps=None, delays=None, in_scale=None, out_scale=None, **kw):
    """I x O full crossbar with independent IRs (configs B and C are this shape)."""
    e = engine_cls(L, N, rs, I, O, **kw)
    e.set_interleaved(0, infmt)
    e.set_interleaved(1, outfmt)
    taps = L * N if taps is None else taps
    irs = {}
    for o in range(O):
        for i in range(I):
            rng = np.random.default_rng(seed + o * I + i)
            h = make_ir(rng, taps, I)
            irs[(o, i)] = h
            c = e.add_coeff(h)
            e.add_filter(in_ch=[i], out_ch=[o], coeff=c,
                         in_scale=[1.0 if in_scale is None else in_scale[o][i]],
                         out_scale=[1.0 if out_scale is None else out_scale[o][i]],
                         delayblocks=0 if delays is None else delays[o][i])
    if hasattr(e, "finalize"):
        e.finalize()
    return e, irs


def raw_blocks(seed, n_blocks, L, n_ch, fmt, amplitude=0.1):
    """seeded noise, frames x channels interleaved, in the raw sample format"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_blocks * L, n_ch)) * amplitude
    if fmt.startswith("FLOAT"):
        raw = x.astype(RAW_NP[fmt])
    else:
        bits = {"S8": 8, "S16_LE": 16, "S24_4LE": 24, "S32_LE": 32}[fmt]
        raw = np.clip(np.round(x * (1 << (bits - 1))), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
        raw = raw.astype(RAW_NP[fmt])
    return [np.ascontiguousarray(raw[b * L:(b + 1) * L]) for b in range(n_blocks)]


def run(engine, blocks):
    outs, sts = [], []
    for b in blocks:
        st, raw = engine.block(b)
        sts.append(st)
        outs.append(raw)
    return sts, outs


def rel_rms(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-300)))


# ------------------------------------------------------------------ generic network builder

def build(engine_cls, spec, **kw):
    """spec: dict(L, N, rs, n_in, n_out, infmt, outfmt, coeffs=[(taps, scale, n_blocks)],
    filters=[dict(in_ch, in_scale, in_f, in_fscale, out_ch, out_scale, coeff, delayblocks,
    crossfade)], safety_limit) -> engine (oracle or HIP: same calls)"""
    e = engine_cls(spec["L"], spec["N"], spec["rs"], spec["n_in"], spec["n_out"], **kw)
    e.set_interleaved(0, spec["infmt"])
    e.set_interleaved(1, spec["outfmt"])
    if spec.get("safety_limit"):
        e.set_safety_limit(spec["safety_limit"])
    for taps, scale, nb in spec.get("coeffs", []):
        e.add_coeff(taps, scale, nb)
    for f in spec["filters"]:
        e.add_filter(**f)
    if hasattr(e, "finalize"):
        e.finalize()
    return e


def samples(raw, fmt):
    return np.frombuffer(raw.tobytes(), RAW_NP[fmt]).astype(np.float64)


def fade_cascade_parts():
    """fade_cascade_network's data: (L, N, blocks, switch block, [ha, hb, hc, hd], input [frames][2])"""
    L, N = 1024, 4
    rng = np.random.default_rng(21)
    irs = [make_ir(rng, L * N - 17 * k, 2) for k in range(4)]
    nblk = 3 * N + 2
    x = rng.standard_normal((nblk * L, 2)) * 0.1
    return L, N, nblk, 2 * N + 1, irs, x


def fade_cascade_network(engine_cls, rs):
    """One network that exercises delay bookkeeping, cascade evaluation and a cross-fade at once,
    and its float64 numpy model (scipy fftconvolve; nothing from oracle/):
       A: in0 -> ha, delayblocks 1            (cascade source)
       B: in1 -> hb                           (cascade source)
       C: 0.25*in0 + 0.5*A - 1.0*B -> hc, cross-fades to hd at block `sw` -> out0 (x 0.8)
       D: in1 -> hd, delayblocks 2 -> out1 and (x -0.5) out0
    Model: delays are whole blocks in front of the convolution (bfrun.c:1600) and cut the filter
    to the N - delay partitions that still fit the ring (cblocks, bfrun.c:1585-1591); a cascade
    adds no delay (convolve_eval, fftw_convolver.c:411-433); in the switch block the output is
    the ramp (1 - n/(L-1)) * old + n/(L-1) * new and afterwards the new taps act on all history
    (fftw_convolver.c:330-368, bfrun.c:1803-1838).  Returns (engine output, model, L, sw)."""
    from scipy.signal import fftconvolve
    dt = np.float32 if rs == 4 else np.float64
    L, N, nblk, sw, irs, x = fade_cascade_parts()
    ha, hb, hc, hd = [h.astype(dt) for h in irs]
    e = engine_cls(L, N, rs, 2, 2)
    e.set_interleaved(0, "FLOAT64_LE")
    e.set_interleaved(1, "FLOAT_LE" if rs == 4 else "FLOAT64_LE")
    ca, cb, cc, cd = [e.add_coeff(h) for h in (ha, hb, hc, hd)]
    fa = e.add_filter(in_ch=[0], coeff=ca, delayblocks=1)
    fb = e.add_filter(in_ch=[1], coeff=cb)
    fc = e.add_filter(in_ch=[0], in_scale=[0.25], in_f=[fa, fb], in_fscale=[0.5, -1.0],
                      out_ch=[0], out_scale=[0.8], coeff=cc, crossfade=True)
    e.add_filter(in_ch=[1], out_ch=[1, 0], out_scale=[1.0, -0.5], coeff=cd, delayblocks=2)
    if hasattr(e, "finalize"):
        e.finalize()
    n = len(x)
    got = []
    for b in range(nblk):
        if b == sw:
            e.set_coeff(fc, cd)
        st, raw = e.block(x[b * L:(b + 1) * L])
        assert st == 0
        got.append(np.frombuffer(raw.tobytes(), dt).reshape(L, 2))
    y = np.concatenate(got).astype(np.float64)

    def conv(sig, h):
        return fftconvolve(np.asarray(sig, np.float64), np.asarray(h, np.float64))[:n]

    def delayed(sig, blocks):
        return np.concatenate([np.zeros(blocks * L), sig[:n - blocks * L]])
    ya = conv(delayed(x[:, 0], 1), ha[:(N - 1) * L])
    yb = conv(x[:, 1], hb)
    in_c = 0.25 * x[:, 0] + 0.5 * ya - yb
    yc_old, yc_new = conv(in_c, hc), conv(in_c, hd)
    w = np.arange(L) / (L - 1.0)
    yc = yc_old.copy()
    s = slice(sw * L, (sw + 1) * L)
    yc[s] = yc_old[s] * (1 - w) + yc_new[s] * w
    yc[(sw + 1) * L:] = yc_new[(sw + 1) * L:]
    yd = conv(delayed(x[:, 1], 2), hd[:(N - 2) * L])
    return y, np.stack([0.8 * yc - 0.5 * yd, yd], axis=1), L, sw


def act(e, a):
    """one run-time call on an oracle or HIP engine: ("coeff", f, c), ("scale", f, io, idx, v),
    ("fscale", f, idx, v) or ("delay", f, d) (xbar_ref.Network.act models the same tuples)"""
    if a[0] == "coeff":
        e.set_coeff(a[1], a[2])
    elif a[0] == "scale":
        e.set_scale(a[1], a[2], a[3], a[4])
    elif a[0] == "fscale":
        e.set_fscale(a[1], a[2], a[3])
    elif a[0] == "delay":
        e.set_delayblocks(a[1], a[2])
    elif a[0] == "subdelay":
        e.set_subdelay(a[1], a[2], a[3])
    elif a[0] == "mute":
        e.set_mute(a[1], a[2], a[3])
    else:
        raise ValueError(a)


# ------------------------------------------------------------------ the channel stage

def build_channels(engine_cls, spec, ch, **kw):
    """a cases.build spec with the channel stage xbar_ref.Channels describes (in_map / out_map,
    in_fmt / out_fmt, delay, sdf_length, subdelay, dither, rate, max_size) -> engine (oracle or HIP).
    mute_from is run-time: mute_actions()"""
    e = engine_cls(spec["L"], spec["N"], spec["rs"], spec["n_in"], spec["n_out"], **kw)
    maps = [list(ch.get("in_map", range(spec["n_in"]))), list(ch.get("out_map", range(spec["n_out"])))]
    for io in range(2):
        if "in_map" in ch or "out_map" in ch:
            e.map_channels(io, maps[io])
        e.set_interleaved_phys(io, ch["in_fmt" if io == 0 else "out_fmt"], max(maps[io]) + 1)
    if ch.get("sdf_length"):
        e.enable_subdelay(ch["sdf_length"])
        for (io, v), value in sorted(ch.get("subdelay", {}).items()):
            e.set_subdelay(io, v, value)
    for (io, v), d in sorted(ch.get("delay", {}).items()):
        e.set_delay(io, v, d)
        e.set_maxdelay(io, v, ch["maxdelay"])
    if spec.get("safety_limit"):
        e.set_safety_limit(spec["safety_limit"])
    for taps, scale, nb in spec.get("coeffs", []):
        e.add_coeff(taps, scale, nb)
    if ch.get("dither"):
        e.enable_dither(list(ch["dither"]), ch.get("rate", 44100), ch.get("max_size", 0))
    for f in spec["filters"]:
        e.add_filter(**f)
    if hasattr(e, "finalize"):
        e.finalize()
    return e


def mute_actions(ch, actions=None):
    """the run-time calls of ch["mute_from"] merged into an action table {block: [tuples]}"""
    out = {t: list(a) for t, a in (actions or {}).items()}
    for (io, v), t in sorted(ch.get("mute_from", {}).items()):
        out.setdefault(t, []).append(("mute", io, v, 1))
    return out


def subdelay_taps(half, rs):
    """-> taps_of(value): the engine's sub-sample filter for `value` hundredths of a sample, as float64
    (bfhip_selftest_subdelay_filter runs on the host; tests/test_nupc_subdelay_abi.py pins it to the
    oracle)"""
    import brutefir_amd as bf
    cache = {}

    def taps_of(value):
        if value not in cache:
            out = np.zeros(2 * half + 1, np.float32 if rs == 4 else np.float64)
            assert bf.lib().bfhip_selftest_subdelay_filter(half, value, rs, out.ctypes.data) == 2 * half + 1
            cache[value] = out.astype(np.float64)
        return cache[value]
    return taps_of


def channel_stage(L, N, rs, outfmt, half, dither=(), loud=1.0, seed=5, rate=300, subdelay=None):
    """(spec, ch, actions): 5 virtual channels a side on 3 physical ones (0,1,0,1 and a 1:1 channel),
    every feature of the channel stage at once.  Member delays 0, 1, L - 1, L and 2L + 3; an input
    and an output member muted from block N + 1 on; with half > 0 sub-sample filters on a shared
    input (37), the 1:1 input read from raw (-99, then 12), a member of a shared output (99, then
    -37) and the 1:1 output in place (0: the pure delay), the changes before block N + 2; subdelay:
    other filtered channels {(io, v): value}, without run-time changes"""
    rng = np.random.default_rng(seed + L)
    n = (N - 1) * L + L // 2 + 1                         # flat taps that end mid-partition
    coeffs = [(rng.standard_normal(n) / np.sqrt(n) / 2, 1.0, 0) for _ in range(10)]
    gain = [1.0, loud, 1.0, loud, 1.0]                   # virtual outputs 1 and 3: physical 1
    filters = [dict(in_ch=[i], out_ch=[o], coeff=2 * i + j, out_scale=[gain[o]])
               for i in range(5) for j, o in enumerate((i, (i + 1) % 5))]
    spec = dict(L=L, N=N, rs=rs, n_in=5, n_out=5, coeffs=coeffs, filters=filters)
    ch = dict(in_map=[0, 1, 0, 1, 2], out_map=[0, 1, 0, 1, 2], in_fmt="S24_LE", out_fmt=outfmt,
              delay={(0, 0): 0, (0, 2): L - 1, (0, 1): 1, (0, 3): 2 * L + 3,
                     (1, 0): L, (1, 2): 1, (1, 1): 0, (1, 3): 2 * L + 3}, maxdelay=3 * L,
              mute_from={(0, 2): N + 1, (1, 3): N + 1}, sdf_length=half,
              subdelay={(0, 0): 37, (0, 4): -99, (1, 1): 99, (1, 4): 0} if subdelay is None else subdelay,
              dither=dither, rate=rate)
    changes = {N + 2: [("subdelay", 1, 1, -37), ("subdelay", 0, 4, 12)]} if half and subdelay is None else None
    if not half:
        ch["subdelay"] = {}
    return spec, ch, mute_actions(ch, changes)


def packed_input(seed, frames, fmts, amplitude=0.2):
    """seeded noise as packed 24-bit frames (nupc_ref.pack) -> the raw stream, uint8"""
    import nupc_ref as nr
    rng = np.random.default_rng(seed)
    q = np.clip(np.round(rng.standard_normal((frames, len(fmts))) * amplitude * (1 << 23)), -(1 << 23), (1 << 23) - 1)
    return nr.pack(q.astype(np.int64), fmts)
