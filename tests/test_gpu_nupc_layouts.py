"""GPU: planar and per-device I/O buffer layouts of the non-uniform convolver
(bfhip_nupc_set_buffer_bytes, include/bfhip_nupc.h): a side's period buffer laid out the way dai.c's
calc_buffer_format lays out any set of devices -- interleaved or not, one sample format each.

Every comparison is device against device and exact.  The yardstick is the interleaved path (held to
the float64 model by tests/test_gpu_nupc_shapes.py and its neighbours): a convolver with a general
layout must give, channel by channel, the sample bytes, overflow structs and status words of an
interleaved convolver fed the same samples and given the same calls.  Where one interleaved frame
cannot carry the side's formats (several widths), the input samples travel in one common width
that load_raw converts to the same reals, and the outputs are compared with one interleaved run
per format."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])               # background segments, 1024-frame input ring
PERIODS = 40                                               # the ring wraps more than twice
IN, OUT = 0, 1
EINVAL, ESTATE = -1, -5


# ---------------------------------------------------------------- layouts and samples

class Side:
    """formats of a side's channels, the period buffer's size, and whether the side opts in"""

    def __init__(self, fmts, nbytes, optin):
        self.fmts, self.nbytes, self.optin = list(fmts), int(nbytes), optin

    def index(self, L0):
        """per channel: [L0][bytes] byte positions of its samples in the period buffer"""
        return [f.byte_offset + (np.arange(L0) * f.sample_spacing * f.bytes)[:, None] + np.arange(f.bytes)[None, :]
                for f in self.fmts]


def planar(hip, names, L0):
    """one non-interleaved device per entry of names (a name, or (name, channels))"""
    devs = []
    for d in names:
        name, n = (d, 1) if isinstance(d, str) else d
        devs.append((name, n, list(range(n)), False))
    fmts, nbytes = hip.period_layout(L0, devs)
    return Side(fmts, nbytes, True)


def inter(hip, name, n, L0, optin=False):
    fmts = hip.interleaved_formats(name, n)
    return Side(fmts, L0 * n * fmts[0].bytes, optin)


def frame(hip, fmts, L0):
    """one interleaved frame of formats that share a width (not opted in)"""
    out = []
    for c, f in enumerate(fmts):
        g = hip.Format(f.isfloat, f.swap, f.bytes, f.sbytes, f.scale, len(fmts), c * f.bytes)
        out.append(g)
    return Side(out, L0 * len(fmts) * fmts[0].bytes, False)


def samples(hip, rng, name, frames, amp=0.3):
    """(raw sample bytes [frames][bytes], the values they encode: int64 or float64)"""
    nbytes, sbytes, isfloat, le = hip.SAMPLE_FORMATS[name]
    x = rng.standard_normal(frames) * amp
    if isfloat:
        v = x.astype("<f4" if nbytes == 4 else "<f8")
        raw = v.view(np.uint8).reshape(frames, nbytes)
        val = v.astype(np.float64)
    else:
        full = 1 << (8 * sbytes - 1)
        val = np.clip(np.round(x * full), -full, full - 1).astype("<i8")
        raw = np.ascontiguousarray(val.view(np.uint8).reshape(frames, 8)[:, :nbytes])
    if not le:
        raw = np.ascontiguousarray(raw[:, ::-1])
    return raw, val


def carrier(hip, rs, name, val):
    """the same values in the common width of realsize rs: (format, raw sample bytes).  Integers go
    as S32_LE (rs 4) or FLOAT64_LE (rs 8) with the scale of the original format, floats as FLOAT_LE
    / FLOAT64_LE: load_raw yields the same real"""
    nbytes, sbytes, isfloat, _ = hip.SAMPLE_FORMATS[name]
    scale = hip.make_format(name).scale
    if rs == 8:
        f = hip.make_format("FLOAT64_LE")
        raw = val.astype("<f8").view(np.uint8).reshape(len(val), 8)
    elif isfloat:
        assert nbytes == 4
        f = hip.make_format("FLOAT_LE")
        raw = val.astype("<f4").view(np.uint8).reshape(len(val), 4)
    else:
        f = hip.make_format("S32_LE")
        raw = val.astype("<i4").view(np.uint8).reshape(len(val), 4)
    f.scale = scale
    return f, np.ascontiguousarray(raw)


def make(hip, sched, rs, sin, sout, filters, pre=None):
    nu = hip.Nupc(sched[0], sched[1], rs, len(sin.fmts), len(sout.fmts))
    for io, s in ((IN, sin), (OUT, sout)):
        for c, f in enumerate(s.fmts):
            nu.set_format(io, c, f)
        if s.optin:
            nu.set_buffer_bytes(io, s.nbytes)
    for i, o, h, scale in filters:
        nu.add_filter(i, o, h, 1.0, scale)
    if pre:
        pre(nu)
    nu.finalize()
    assert nu.buffer_bytes(IN) == sin.nbytes and nu.buffer_bytes(OUT) == sout.nbytes
    return nu


def taps_for(n_in, n_out, total, seed, loud=None):
    """(input, output, taps, out_scale): two filters per output (from inputs o and o + 1); output
    `loud` is 40x louder"""
    rng = np.random.default_rng(seed)
    n = min(total, 3000)
    env = np.exp(-np.arange(n) / 400.0)
    fl = []
    for o in range(n_out):
        for i in sorted({o % n_in, (o + 1) % n_in}):
            fl.append((i, o, rng.standard_normal(n) * env / 12.0, 40.0 if o == loud else 1.0))
    return fl


class Run:
    pass


def run(hip, nu, sin, sout, chans, periods, L0, actions=None, dev=False):
    """feed `chans` ([channel] -> [frames][bytes]) through block() (or block_dev()).  Returns per
    output channel its sample bytes [frames][bytes], the status words, the overflow structs after
    every period, and the output bytes no channel owns."""
    ii, oi = sin.index(L0), sout.index(L0)
    owned = np.zeros(sout.nbytes, bool)
    for ix in oi:
        assert not owned[ix].any()
        owned[ix] = True
    n_out = len(sout.fmts)
    r = Run()
    r.out = [[] for _ in range(n_out)]
    r.st, r.of, r.unowned = [], [], []
    ovf = (hip.Overflow * n_out)(*[hip.Overflow(0, 0, 0.0, 1.0 if f.isfloat else float((1 << (8 * f.sbytes - 1)) - 1))
                                   for f in sout.fmts])
    if dev:
        import torch
    for p in range(periods):
        if actions and p in actions:
            actions[p](nu)
        buf = np.full(sin.nbytes, 0x5A, np.uint8)                 # unowned input bytes are never read as samples
        for c, ix in enumerate(ii):
            buf[ix] = chans[c][p * L0:(p + 1) * L0]
        if dev:
            din = torch.from_numpy(buf).cuda()
            dout = torch.full((sout.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            nu.block_dev(din, dout)
            st = nu.sync()
            assert np.array_equal(din.cpu().numpy(), buf), p      # the caller's input is never modified
            y = dout.cpu().numpy()
            r.of.append([nu.overflow(c).astuple() for c in range(n_out)])
        else:
            st, y = nu.block(buf, ovf)
            r.of.append([o.astuple() for o in ovf])
        assert y.size == sout.nbytes
        r.st.append(st)
        r.unowned.append(y[~owned].copy())
        for c, ix in enumerate(oi):
            r.out[c].append(y[ix])
    r.out = [np.concatenate(o) for o in r.out]
    r.unowned = np.concatenate(r.unowned) if r.unowned else np.zeros(0, np.uint8)
    return r


def same(a, b):
    """runs a and b agree in every channel's bytes, every overflow struct and every status word"""
    assert a.st == b.st
    assert len(a.out) == len(b.out)
    for c in range(len(a.out)):
        assert np.array_equal(a.out[c], b.out[c]), (c, int(np.argmax(np.any(a.out[c] != b.out[c], axis=1))))
    assert a.of == b.of


# ---------------------------------------------------------------- 1. planar equals interleaved

@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("name", ["S16_LE", "S24_LE", "S32_LE", "FLOAT_LE", "FLOAT64_LE", "S24_BE"])
def test_planar_equals_interleaved(hip, name, rs):
    """both sides one non-interleaved device, 3 x 3, two filters per output, output 2 loud (it clips:
    integer formats at full scale, floats beyond +-1.0); the overflow structs are reset once on the
    way.  64-frame planes fill a multiple of 32 bytes, so the planar output buffer is declared 40
    bytes longer than its planes: bytes no channel owns, which block() returns as zero"""
    L0, T = 64, PERIODS * 64
    rng = np.random.default_rng(len(name) * 7 + rs)
    chans = [samples(hip, rng, name, T)[0] for _ in range(3)]
    fl = taps_for(3, 3, 3968, 5, loud=2)
    acts = {17: lambda nu: nu.reset_overflow()}
    res = []
    for mk in (lambda: planar(hip, [(name, 3)], L0), lambda: inter(hip, name, 3, L0)):
        sin, sout = mk(), mk()
        if sout.optin:
            sout.nbytes += 40
        nu = make(hip, SMALL, rs, sin, sout, fl)
        res.append(run(hip, nu, sin, sout, chans, PERIODS, L0, acts))
        res[-1].final = [nu.overflow(c).astuple() for c in range(3)]
    same(res[0], res[1])
    assert res[0].final == res[1].final == res[0].of[-1]
    assert res[0].unowned.size == PERIODS * 40 and not res[0].unowned.any()
    assert res[1].of[16][2][0] > 0 and res[1].of[-1][2][0] > 0     # it clipped before and after the reset


# ---------------------------------------------------------------- 2. - 4., 8.: mixed devices

MIXED_IN = [("S16_LE", 3, [2, 0], True), ("FLOAT_LE", 2, [0, 1], False), ("S24_LE", 1, [0], False)]
MIXED_IN_NAMES = ["S16_LE", "S16_LE", "FLOAT_LE", "FLOAT_LE", "S24_LE"]
MIXED_OUT = [("S16_LE", 2, [0, 1], True), ("S24_4LE", 1, [0], False), ("FLOAT_LE", 1, [0], False),
             ("S32_LE", 1, [0], False)]
MIXED_OUT_NAMES = ["S16_LE", "S16_LE", "S24_4LE", "FLOAT_LE", "S32_LE"]
INT_OUT = [("S16_LE", 2, [0, 1], True), ("S24_4LE", 1, [0], False), ("S32_LE", 1, [0], False)]
INT_OUT_NAMES = ["S16_LE", "S16_LE", "S24_4LE", "S32_LE"]


def mixed_inputs(hip, rs, L0, T, seed):
    """the worked example's input layout at L0, its samples, and the carrier side with its samples"""
    rng = np.random.default_rng(seed)
    fmts, nbytes = hip.period_layout(L0, MIXED_IN)
    sin = Side(fmts, nbytes, True)
    raw, car_f, car_raw = [], [], []
    for name in MIXED_IN_NAMES:
        b, v = samples(hip, rng, name, T)
        f, cb = carrier(hip, rs, name, v)
        raw.append(b); car_f.append(f); car_raw.append(cb)
    return sin, raw, frame(hip, car_f, L0), car_raw


def delay_plan(n_in, n_out, L0, three_byte_in):
    """per-channel maxdelay / delay on both sides and the run-time calls, as (pre, actions)"""
    spec_in = [(L0 - 5, -1), (3 * L0 + 7, 4 * L0), (0, 2 * L0), (L0, -1), (L0 - 9, L0)][:n_in]
    spec_out = [(2 * L0 + 5, -1), (10, 3 * L0), (L0, L0), (0, -1), (L0 + 1, 2 * L0)][:n_out]
    assert spec_in[three_byte_in][0] <= L0                       # the packed 3-byte channel: a delay <= L0

    def pre(nu):
        for io, spec in ((IN, spec_in), (OUT, spec_out)):
            for ch, (d, m) in enumerate(spec):
                nu.set_maxdelay(io, ch, m)
                nu.set_delay(io, ch, d)
    acts = {
        6: lambda nu: (nu.set_delay(IN, 1, 4 * L0), nu.set_delay(OUT, 1, 3 * L0 - 1)),         # increases
        11: lambda nu: (nu.set_mute(IN, 0, 1), nu.set_mute(OUT, n_out - 1, 1), nu.set_mute(IN, three_byte_in, 1)),
        19: lambda nu: (nu.set_delay(IN, 1, 17), nu.set_delay(OUT, 1, 3), nu.set_delay(IN, 2, L0 + 30)),   # decreases
        24: lambda nu: (nu.set_mute(IN, 0, 0), nu.set_mute(OUT, n_out - 1, 0), nu.set_mute(IN, three_byte_in, 0)),
        31: lambda nu: nu.set_mute(OUT, 0, 1),
    }
    return pre, acts


def mixed_case(hip, rs, out_devs, out_names, delays=False, dither=False, dev=False, periods=PERIODS):
    """the general convolver (mixed devices on both sides) against one interleaved convolver per
    output format, whose inputs carry the same values in one common width"""
    L0, T = 64, periods * 64
    sin, raw, scar, car_raw = mixed_inputs(hip, rs, L0, T, 11 + rs)
    n_out = len(out_names)
    fmts, nbytes = hip.period_layout(L0, out_devs)
    sout = Side(fmts, nbytes, True)
    fl = taps_for(5, n_out, 3968, 9, loud=1)
    dpre, acts = delay_plan(5, n_out, L0, 4) if delays else (None, None)

    def pre(nu):
        if dither:
            nu.enable_dither(list(range(n_out)), 300)
        if dpre:
            dpre(nu)
    g = run(hip, make(hip, SMALL, rs, sin, sout, fl, pre), sin, sout, raw, periods, L0, acts, dev=dev)
    clipped = 0
    for name in sorted(set(out_names)):
        so = inter(hip, name, n_out, L0)
        ref = run(hip, make(hip, SMALL, rs, scar, so, fl, pre), scar, so, car_raw, periods, L0, acts)
        chs = [c for c in range(n_out) if out_names[c] == name]
        for c in chs:
            assert np.array_equal(g.out[c], ref.out[c]), (name, c)
            assert [o[c] for o in g.of] == [o[c] for o in ref.of], (name, c)
            clipped += ref.of[-1][c][0]
        assert all(s == 0 for s in ref.st)
    assert all(s == 0 for s in g.st)
    assert clipped > 0                                            # the loud S16 output clips
    return g, sin, sout


@pytest.mark.parametrize("rs", [4, 8])
def test_mixed_devices_on_the_input_side(hip, rs):
    """interleaved S16_LE (3 open, selection [2, 0]) + two FLOAT_LE planes + one packed S24_LE
    plane against carriers of one width in interleaved frames; same filters, same output bytes"""
    L0, T = 64, PERIODS * 64
    sin, raw, scar, car_raw = mixed_inputs(hip, rs, L0, T, 2 + rs)
    assert [(f.byte_offset, f.sample_spacing) for f in sin.fmts] == [(4, 3), (0, 3), (384, 1), (640, 1), (896, 1)]
    assert sin.nbytes == 1088
    outname = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    fl = taps_for(5, 3, 3968, 4)
    so = inter(hip, outname, 3, L0)
    a = run(hip, make(hip, SMALL, rs, sin, so, fl), sin, so, raw, PERIODS, L0)
    b = run(hip, make(hip, SMALL, rs, scar, so, fl), scar, so, car_raw, PERIODS, L0)
    same(a, b)
    assert a.out[0].any()


@pytest.mark.parametrize("rs", [4, 8])
def test_mixed_devices_on_the_output_side(hip, rs):
    g, _, sout = mixed_case(hip, rs, MIXED_OUT, MIXED_OUT_NAMES)
    assert sout.nbytes == 256 + 256 + 256 + 256 and not g.unowned.any()


@pytest.mark.parametrize("rs", [4, 8])
def test_mixed_integer_outputs_all_dithered(hip, rs):
    """every output dithered in the general run and in the per-format runs: the dither slots have
    the same ranks, so the bytes are identical"""
    mixed_case(hip, rs, INT_OUT, INT_OUT_NAMES, dither=True)


@pytest.mark.parametrize("rs", [4, 8])
def test_delay_and_mute_on_general_layouts(hip, rs):
    """per-channel maxdelay / delay on both sides (a delay <= L0 on the packed 3-byte plane), a
    run-time increase and decrease and mutes toggled at fixed periods: equal to the carrier and
    per-format runs given the same calls"""
    mixed_case(hip, rs, MIXED_OUT, MIXED_OUT_NAMES, delays=True)


def test_delay_jobs_of_more_than_one_launch(hip):
    """33 planar S16_LE inputs, all delayed, one output: more jobs than one launch carries"""
    L0, periods, n = 64, 12, 33
    rng = np.random.default_rng(33)
    chans = [samples(hip, rng, "S16_LE", periods * L0)[0] for _ in range(n)]
    h = [np.random.default_rng(100 + i).standard_normal(200) / 40.0 for i in range(n)]
    fl = [(i, 0, h[i], 1.0) for i in range(n)]

    def pre(nu):
        for c in range(n):
            nu.set_maxdelay(IN, c, 3 * L0)
            nu.set_delay(IN, c, (7 * c) % (3 * L0) + 1)
    acts = {5: lambda nu: [nu.set_delay(IN, c, (11 * c) % (3 * L0)) for c in range(n)],
            8: lambda nu: [nu.set_mute(IN, c, c % 3 == 0) for c in range(n)]}
    res = []
    for sin in (planar(hip, [("S16_LE", n)], L0), inter(hip, "S16_LE", n, L0)):
        so = inter(hip, "FLOAT_LE", 1, L0)
        res.append(run(hip, make(hip, SMALL, 4, sin, so, fl, pre), sin, so, chans, periods, L0, acts))
    same(res[0], res[1])
    assert res[0].out[0].any()


# ---------------------------------------------------------------- 5. sub-sample delay on a planar side

@pytest.mark.parametrize("rs", [4, 8])
def test_subdelay_on_planar_sides(hip, rs):
    """sdf_length 31, filters on inputs 0 and 2 and on outputs 1 and 2, values changed at run time;
    the unfiltered channels get their 31 whole frames through lines sized per channel"""
    L0, T = 64, PERIODS * 64
    chans = [samples(hip, np.random.default_rng(70 + c), "S24_LE", T)[0] for c in range(3)]
    fl = taps_for(3, 3, 3968, 6, loud=0)

    def pre(nu):
        nu.enable_subdelay(31)
        nu.set_subdelay(IN, 0, 37); nu.set_subdelay(IN, 2, -80)
        nu.set_subdelay(OUT, 1, 5); nu.set_subdelay(OUT, 2, 99)
    acts = {9: lambda nu: (nu.set_subdelay(IN, 0, -12), nu.set_subdelay(OUT, 2, 0)),
            27: lambda nu: nu.set_subdelay(IN, 2, 61)}
    res = []
    for mk in (lambda: planar(hip, [("S24_LE", 3)], L0), lambda: inter(hip, "S24_LE", 3, L0)):
        sin, sout = mk(), mk()
        res.append(run(hip, make(hip, SMALL, rs, sin, sout, fl, pre), sin, sout, chans, PERIODS, L0, acts))
    same(res[0], res[1])
    assert res[1].of[-1][0][0] > 0


# ---------------------------------------------------------------- 6. everything at once

@pytest.mark.parametrize("rs", [4, 8])
def test_switch_gains_ramp_and_dither_planar_against_interleaved(hip, rs):
    """second sets with a switch and a 100-frame cross-fade, a per-filter gain switch, an output gain
    ramp and dither inside the 40 periods: identical bytes and identical switch_frame"""
    L0, T = 64, PERIODS * 64
    chans = [samples(hip, np.random.default_rng(80 + c + rs), "S24_LE", T)[0] for c in range(3)]
    fl = taps_for(3, 3, 3968, 8, loud=2)

    def pre(nu):
        nu.enable_dither([0, 1, 2], 300)
        nu.reserve_filter_gain()
        for f, (_, _, h, _) in enumerate(fl):
            nu.add_coeff(f, -0.5 * h[::-1].copy())

    def switch(nu):
        nu.set_crossfade(100)
        for f in range(len(fl)):
            nu.set_coeff(f, 1)

    def gains(nu):
        assert not nu.switch_busy()
        nu.set_filter_gain(0, 0.25)
        nu.set_filter_gain(3, -1.5)

    def ramp(nu):
        nu.set_gain_ramp(200)
        nu.set_output_gain(0, 0.3)
        nu.set_output_gain(2, 1.7)
    acts = {3: ramp, 7: switch, 30: gains}
    res, frames = [], []
    for k in range(2):
        mk = (lambda n: planar(hip, [(n, 3)], L0)) if k == 0 else (lambda n: inter(hip, n, 3, L0))
        sin, sout = mk("S24_LE"), mk("S16_LE")
        nu = make(hip, SMALL, rs, sin, sout, fl, pre)
        res.append(run(hip, nu, sin, sout, chans, PERIODS, L0, acts))
        frames.append(nu.switch_frame())
    same(res[0], res[1])
    assert frames[0] == frames[1] >= 30 * L0


# ---------------------------------------------------------------- 7. block-length extremes

@pytest.mark.parametrize("rs", [4, 8])
def test_eight_frame_periods_with_unaligned_planes(hip, rs):
    """L0 = 8: packed S24_LE planes are 24 bytes, so two of three start at an unaligned offset"""
    L0, periods, sched = 8, 60, ([8, 16, 32], [2, 2, 2])
    chans = [samples(hip, np.random.default_rng(90 + c), "S24_LE", periods * L0)[0] for c in range(3)]
    fl = taps_for(3, 3, 112, 12, loud=2)
    res = []
    for mk in (lambda: planar(hip, [("S24_LE", 3)], L0), lambda: inter(hip, "S24_LE", 3, L0)):
        sin, sout = mk(), mk()
        if sin.optin:
            assert [f.byte_offset for f in sin.fmts] == [0, 24, 48] and sin.nbytes == 96
        res.append(run(hip, make(hip, sched, rs, sin, sout, fl), sin, sout, chans, periods, L0))
    same(res[0], res[1])
    assert not res[0].unowned.any() and res[0].unowned.size == periods * 24


@pytest.mark.parametrize("rs", [4, 8])
def test_512_frame_periods_with_subdelay(hip, rs):
    """more than 256 frames per workgroup in the conversion, and the FIR tile"""
    L0, periods, sched = 512, 6, ([512, 1024], [2, 2])
    chans = [samples(hip, np.random.default_rng(95 + c), "FLOAT_LE", periods * L0)[0] for c in range(2)]
    fl = taps_for(2, 2, 3072, 13)

    def pre(nu):
        nu.enable_subdelay(31)
        nu.set_subdelay(IN, 1, 44)
        nu.set_subdelay(OUT, 0, -7)
    res = []
    for mk in (lambda: planar(hip, [("FLOAT_LE", 2)], L0), lambda: inter(hip, "FLOAT_LE", 2, L0)):
        sin, sout = mk(), mk()
        res.append(run(hip, make(hip, sched, rs, sin, sout, fl, pre), sin, sout, chans, periods, L0))
    same(res[0], res[1])
    assert res[0].out[1].any()


# ---------------------------------------------------------------- 8. block_dev

@pytest.mark.parametrize("rs", [4, 8])
def test_block_dev_on_general_layouts(hip, rs):
    """device buffers, the output prefilled with 0xA5: the owned bytes are block()'s, the unowned
    ones are untouched, and the caller's input is unchanged with an input delay and a mute in force
    (run() checks it every period)"""
    L0, periods = 64, 30
    sin, raw, _, _ = mixed_inputs(hip, rs, L0, periods * L0, 21)
    fmts, nbytes = hip.period_layout(L0, MIXED_OUT)
    sout = Side(fmts, nbytes + 64, True)                          # 64 bytes nobody owns
    fl = taps_for(5, 5, 3968, 9, loud=1)
    dpre, acts = delay_plan(5, 5, L0, 4)
    a = run(hip, make(hip, SMALL, rs, sin, sout, fl, dpre), sin, sout, raw, periods, L0, acts)
    b = run(hip, make(hip, SMALL, rs, sin, sout, fl, dpre), sin, sout, raw, periods, L0, acts, dev=True)
    same(b, a)
    assert a.unowned.size == periods * 64 and not a.unowned.any()
    assert b.unowned.size == periods * 64 and np.all(b.unowned == 0xA5)


# ---------------------------------------------------------------- 9. argument and state rules

def _bare(hip, n_in=2, n_out=2, rs=4):
    nu = hip.Nupc(SMALL[0], SMALL[1], rs, n_in, n_out)
    for i in range(n_in):
        nu.add_filter(i, i % n_out, np.ones(8))
    return nu


def _finalize_code(hip, nu):
    return hip.lib().bfhip_nupc_finalize(nu.h), hip.lib().bfhip_nupc_last_error().decode()


@pytest.mark.parametrize("io", [IN, OUT])
def test_overlapping_channels_are_refused(hip, io):
    nu = _bare(hip)
    nu.set_format(io, 0, hip.make_format("S16_LE", 1, 0))
    nu.set_format(io, 1, hip.make_format("S16_LE", 1, 126))       # its first sample is the other's last
    nu.set_buffer_bytes(io, 512)
    code, msg = _finalize_code(hip, nu)
    assert code == EINVAL and ("output 1" if io == OUT else "input 1") in msg and "overlap" in msg


def test_layout_argument_and_state_rules(hip):
    L = hip.lib()
    nu = _bare(hip)
    assert L.bfhip_nupc_set_buffer_bytes(nu.h, IN, 0) == EINVAL
    assert L.bfhip_nupc_set_buffer_bytes(nu.h, IN, -5) == EINVAL
    assert L.bfhip_nupc_set_buffer_bytes(nu.h, 2, 64) == EINVAL
    assert L.bfhip_nupc_buffer_bytes(nu.h, IN) == ESTATE          # before finalize
    assert L.bfhip_nupc_buffer_bytes(nu.h, 7) == EINVAL
    # a last sample past the buffer
    nu.set_format(IN, 0, hip.make_format("S24_LE", 1, 0))
    nu.set_format(IN, 1, hip.make_format("S24_LE", 1, 192))
    nu.set_buffer_bytes(IN, 383)
    code, msg = _finalize_code(hip, nu)
    assert code == EINVAL and "input 1" in msg
    # the same layout in 384 bytes is fine; then the state rules
    nu = _bare(hip)
    nu.set_format(IN, 0, hip.make_format("S24_LE", 1, 0))
    nu.set_format(IN, 1, hip.make_format("S24_LE", 1, 192))
    nu.set_buffer_bytes(IN, 384)
    nu.finalize()
    assert L.bfhip_nupc_set_buffer_bytes(nu.h, IN, 384) == ESTATE
    assert nu.buffer_bytes(IN) == 384
    assert nu.buffer_bytes(OUT) == 64 * 2 * 4                     # did not opt in: L0 * spacing * bytes
    # sample_spacing 0, and a negative byte_offset
    for f in (hip.make_format("S16_LE", 0, 0), hip.make_format("S16_LE", 1, -2)):
        nu = _bare(hip)
        nu.set_format(OUT, 0, hip.make_format("S16_LE", 1, 128))
        nu.set_format(OUT, 1, f)
        nu.set_buffer_bytes(OUT, 512)
        code, msg = _finalize_code(hip, nu)
        assert code == EINVAL and "output 1" in msg


def test_mixed_layout_without_the_opt_in_fails_as_before(hip):
    nu = _bare(hip)
    fmts, _ = hip.period_layout(64, [("S16_LE", 1, [0], False), ("FLOAT_LE", 1, [0], False)])
    for c, f in enumerate(fmts):
        nu.set_format(IN, c, f)
    code, msg = _finalize_code(hip, nu)
    assert code == EINVAL and msg == "nupc: all channels of a side must share one interleaved frame layout"


def test_an_input_side_that_opts_in_has_at_most_256_channels(hip):
    n = 257
    nu = hip.Nupc([64], [1], 4, n, 1)
    fmts, nbytes = hip.period_layout(64, [("S16_LE", n, list(range(n)), False)])
    for c, f in enumerate(fmts):
        nu.set_format(IN, c, f)
    nu.set_buffer_bytes(IN, nbytes)
    nu.add_filter(0, 0, np.ones(4))
    code, msg = _finalize_code(hip, nu)
    assert code == EINVAL and "256" in msg


@pytest.mark.parametrize("rs", [4, 8])
def test_opting_in_with_an_interleaved_layout_changes_no_byte(hip, rs):
    L0, periods = 64, 20
    chans = [samples(hip, np.random.default_rng(40 + c), "S16_LE", periods * L0)[0] for c in range(2)]
    fl = taps_for(2, 3, 3968, 14, loud=1)
    res = []
    for optin in (True, False):
        sin, sout = inter(hip, "S16_LE", 2, L0, optin), inter(hip, "S24_4LE", 3, L0, optin)
        res.append(run(hip, make(hip, SMALL, rs, sin, sout, fl), sin, sout, chans, periods, L0))
    same(res[0], res[1])
    assert res[1].of[-1][1][0] > 0
