"""GPU: per-channel sub-sample delay on the inputs and outputs of the non-uniform convolver
(bfhip_nupc_enable_subdelay / _set_subdelay / _get_subdelay, include/bfhip_nupc.h).  The
reference filters a channel's time-domain reals once per period (bfrun.c:1497-1531, 1921-1925,
delay.c:416-442); with a period of L0 frames the convolver must produce exactly that.

Two kinds of reference.  Value 0 is a unit pulse at tap sdf_length, so a convolver filtered at 0
equals, byte for byte, a twin without sub-delay whose channels have an integer delay of sdf_length.
Fractional values are held to a float64 model built from the taps the library itself reports
(bfhip_selftest_subdelay_filter, pinned to the oracle by tests/test_nupc_subdelay_abi.py): decode,
FIR per period on unfiltered history, nupc_ref.convolve, FIR on the outputs, nupc_ref.encode.

Bars.  Float outputs: the project's parity bars, relative RMS 1e-5 (float32 realsize) and 1e-12
(float64).  Integer outputs: no sample more than one count from the model; that can only be asked
where the working precision resolves a count, so float32 runs use S16_LE (1e-5 of a 16-bit signal
is a fraction of a count; of a 24- or 32-bit one it is tens to thousands) and float64 runs the
wider formats."""
import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_ref as nr
from nupc_chain_ref import fir as _fir

pytestmark = pytest.mark.gpu
SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])     # a zero-slack segment, background segments, L0 = 64
BIG = ([512, 1024], [2, 2])                     # L0 above the workgroup size
IN, OUT = 0, 1
EINVAL, ESTATE = -1, -5
UNDEF = -100


def _raw(rng, fmt, frames, n_ch, amp=0.1):
    """random raw frames; amp may be per frame.  No sample is exactly zero."""
    nbytes, sbytes, isfloat, _ = bo.SAMPLE_FORMATS[fmt]
    x = rng.standard_normal((frames, n_ch)) * np.reshape(amp, (-1, 1))
    if isfloat:
        return x.astype(np.float32 if nbytes == 4 else np.float64).view(np.uint8).reshape(frames, -1)
    full = 1 << (8 * sbytes - 1)
    v = np.clip(np.round(x * full), -full, full - 1)
    v[v == 0] = 1
    v = v.astype("<i8")
    return np.ascontiguousarray(v.view(np.uint8).reshape(frames, n_ch, 8)[:, :, :nbytes]).reshape(frames, -1)


def _nupc(hip, rs, n_ch, infmt, outfmt, sched=SMALL, seed=7, gain=1.0, sets=False, dither=None):
    """a convolver with two filters per output; returns it and the model's filter lists (set 0 and,
    with sets=True, set 1 of every filter) in the taps' working precision"""
    nu = hip.Nupc(sched[0], sched[1], rs, n_ch, n_ch)
    nu.set_interleaved(0, infmt)
    nu.set_interleaved(1, outfmt)
    if dither:
        nu.enable_dither(dither, 300)
    rng = np.random.default_rng(seed)
    n = min(nu.taps, 3000)
    env = np.exp(-np.arange(n) / 400.0)
    f0, f1 = [], []
    for o in range(n_ch):
        for i in (o, (o + 1) % n_ch):
            h = (rng.standard_normal(n) * env * gain / 12.0).astype(nu.dt)
            nu.add_filter(i, o, h)
            f0.append((i, o, h.astype(np.float64), 1.0, 1.0))
    if sets:
        for f, (i, o, h, _, _) in enumerate(f0):
            h1 = (-0.5 * h[::-1]).astype(nu.dt)
            assert nu.add_coeff(f, h1) == 1
            f1.append((i, o, h1.astype(np.float64), 1.0, 1.0))
    return nu, f0, f1


def _ovf(outfmt, n_ch, hip):
    nbytes, sbytes, isfloat, _ = bo.SAMPLE_FORMATS[outfmt]
    mx = 1.0 if isfloat else float((1 << (8 * sbytes - 1)) - 1)
    return (hip.Overflow * n_ch)(*[hip.Overflow(0, 0, 0.0, mx) for _ in range(n_ch)])


def _run(nu, x, L0, periods, events=None, ovf=None):
    """periods block calls; events: {period: callable} run before that period's call"""
    out, sts = [], []
    for p in range(periods):
        if events and p in events:
            events[p]()
        st, y = nu.block(x[p * L0:(p + 1) * L0], ovf)
        sts.append(st)
        out.append(y)
    return np.concatenate(out), sts


def _fmts(name, n_ch):
    return bo.interleaved_formats(name, n_ch)


def _check(got_raw, want_raw, outfmt, n_ch, frames, rs):
    fm = _fmts(outfmt, n_ch)
    if bo.SAMPLE_FORMATS[outfmt][2]:
        g, w = nr.decode(got_raw, fm, frames), nr.decode(want_raw, fm, frames)
        for c in range(n_ch):
            err = cases.rel_rms(g[:, c], w[:, c])
            print("rel rms ch %d: %.3g" % (c, err))
            assert err <= (1e-5 if rs == 4 else 1e-12), (c, err)
    else:
        d = np.abs(nr.ints(got_raw, fm, frames) - nr.ints(want_raw, fm, frames))
        print("max count difference %d, samples off %d" % (d.max(), (d > 0).sum()))
        assert d.max() <= 1, d.max()


def _const(v, periods):
    return None if v is None else [v] * periods


def _model(hip, x_raw, infmt, outfmt, n_ch, rs, L0, periods, half, filters, vin, vout, in_mute=None, gain=None,
           blend=None, dither=()):
    """vin / vout: per channel a list of per-period values, or None (no filter; on a side where
    some channel has one that is `half` frames of delay).  in_mute: [frames][n_ch] bool applied to
    the decoded input.  gain: [frames][n_ch].  blend: (filters_new, t_sw, F)."""
    n = periods * L0
    xr = nr.decode(x_raw.ravel(), _fmts(infmt, n_ch), n)
    if in_mute is not None:
        xr = np.where(in_mute, 0.0, xr)
    if any(v is not None for v in vin):
        xr = np.stack([_fir(xr[:, c], vin[c], half, rs, L0) for c in range(n_ch)], axis=1)
    y = nr.convolve(xr, filters, n_ch)
    if blend:
        y = nr.crossfade(y, nr.convolve(xr, blend[0], n_ch), blend[1], blend[2])
    if gain is not None:
        y = y * gain
    if any(v is not None for v in vout):
        y = np.stack([_fir(y[:, c], vout[c], half, rs, L0) for c in range(n_ch)], axis=1)
    raw, of, _ = nr.encode(y, _fmts(outfmt, n_ch), L0, dither=tuple(dither), rate=300)
    return raw


# ---------------------------------------------------------------- 1. exact, input side

@pytest.mark.parametrize("rs,infmt,sched,half", [
    (4, "S16_LE", SMALL, 31), (4, "S24_LE", SMALL, 15), (4, "S32_LE", SMALL, 7), (4, "FLOAT_LE", SMALL, 31),
    (4, "FLOAT64_LE", BIG, 31), (8, "S16_LE", BIG, 15), (8, "S24_LE", SMALL, 31), (8, "S32_LE", BIG, 7),
    (8, "FLOAT_LE", SMALL, 7), (8, "FLOAT64_LE", SMALL, 31), (4, "S24_LE", BIG, 7)])
def test_inputs_filtered_at_zero_equal_an_integer_delay(hip, rs, infmt, sched, half):
    """every input has a filter at value 0: the bytes of a twin whose inputs have an integer delay
    of sdf_length"""
    n_ch, periods, L0 = 3, 40, sched[0][0]
    outfmt = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    a, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    b, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    a.enable_subdelay(half)
    for ch in range(n_ch):
        a.set_subdelay(IN, ch, 0)
        b.set_delay(IN, ch, half)
    a.finalize()
    b.finalize()
    x = _raw(np.random.default_rng(rs + half), infmt, periods * L0, n_ch)
    for p in range(periods):
        sa, ya = a.block(x[p * L0:(p + 1) * L0])
        sb, yb = b.block(x[p * L0:(p + 1) * L0])
        assert sa == sb == 0
        assert np.array_equal(ya, yb), p
    assert ya.any()
    assert [a.get_subdelay(IN, ch) for ch in range(n_ch)] == [0] * n_ch
    assert [a.get_delay(IN, ch) for ch in range(n_ch)] == [0] * n_ch


# ---------------------------------------------------------------- 2. exact, mixed side

@pytest.mark.parametrize("rs,infmt,sched,half", [(4, "S16_LE", SMALL, 31), (8, "S24_LE", SMALL, 15),
                                                 (4, "FLOAT_LE", BIG, 7), (8, "FLOAT64_LE", BIG, 31)])
def test_unfiltered_inputs_get_sdf_length_frames_of_delay(hip, rs, infmt, sched, half):
    """one input filtered at 0, the others without a filter: they follow sdf_length whole frames
    later through their delay lines.  Input 1 has a positive maxdelay, its own delay and a
    run-time change; the twin's line carries sdf_length more in all three."""
    n_ch, periods, L0 = 3, 40, sched[0][0]
    outfmt = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    a, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    b, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    a.enable_subdelay(half)
    a.set_subdelay(IN, 0, 0)
    a.set_maxdelay(IN, 1, 3 * L0)
    a.set_delay(IN, 1, 5)
    b.set_delay(IN, 0, half)
    b.set_maxdelay(IN, 1, 3 * L0 + half)
    b.set_delay(IN, 1, 5 + half)
    b.set_delay(IN, 2, half)
    a.finalize()
    b.finalize()
    assert (a.get_delay(IN, 0), a.get_delay(IN, 1), a.get_delay(IN, 2)) == (0, 5, 0)
    x = _raw(np.random.default_rng(3 * rs + half), infmt, periods * L0, n_ch)
    for p in range(periods):
        if p == 15:
            a.set_delay(IN, 1, L0 + 9)
            b.set_delay(IN, 1, L0 + 9 + half)
        if p == 28:
            a.set_delay(IN, 1, 3 * L0 + 1)            # above maxdelay: ignored by both
            b.set_delay(IN, 1, 3 * L0 + 1 + half)
            a.set_delay(IN, 2, 7)                     # a fixed line stays fixed
        sa, ya = a.block(x[p * L0:(p + 1) * L0])
        sb, yb = b.block(x[p * L0:(p + 1) * L0])
        assert sa == sb == 0
        assert np.array_equal(ya, yb), p
    assert (a.get_delay(IN, 1), a.get_delay(IN, 2)) == (L0 + 9, 0)
    assert a.get_subdelay(IN, 1) == UNDEF


# ---------------------------------------------------------------- 3. exact, output side

@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("rs,outfmt,sched,half", [
    (4, "S16_LE", SMALL, 31), (8, "S24_LE", SMALL, 15), (8, "S32_LE", SMALL, 7), (4, "FLOAT_LE", SMALL, 31),
    (8, "FLOAT64_LE", SMALL, 31), (4, "S16_LE", BIG, 31), (8, "S24_LE", BIG, 7)])
def test_outputs_filtered_at_zero_equal_an_integer_delay(hip, rs, outfmt, sched, half, mixed):
    """a unit-pulse FIR in front of the quantiser equals the integer delay behind it, byte for
    byte; mixed: only output 0 has a filter, output 1 a changeable line with a run-time change.
    Overflow counters: the filtered convolver counts a sample sdf_length frames after the twin
    does, so the input is loud (and clips) in the first periods only and is 40 dB down for the
    last 45; by the last period both have counted every loud sample, and the counters are equal."""
    n_ch, periods, L0 = 3, 60, sched[0][0]
    infmt = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    a, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, sched, gain=6.0)
    b, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, sched, gain=6.0)
    a.enable_subdelay(half)
    for ch in range(n_ch):
        if not mixed or ch == 0:
            a.set_subdelay(OUT, ch, 0)
        b.set_delay(OUT, ch, half)
    if mixed:
        a.set_maxdelay(OUT, 1, 2 * L0)
        a.set_delay(OUT, 1, 3)
        b.set_maxdelay(OUT, 1, 2 * L0 + half)
        b.set_delay(OUT, 1, 3 + half)
    a.finalize()
    b.finalize()
    oa, ob = _ovf(outfmt, n_ch, hip), _ovf(outfmt, n_ch, hip)
    amp = np.where(np.arange(periods * L0) < 15 * L0, 0.3, 0.003)
    x = _raw(np.random.default_rng(11 + rs + half), infmt, periods * L0, n_ch, amp)
    for p in range(periods):
        if mixed and p == 20:
            a.set_delay(OUT, 1, L0 + 2)
            b.set_delay(OUT, 1, L0 + 2 + half)
        sa, ya = a.block(x[p * L0:(p + 1) * L0], oa)
        sb, yb = b.block(x[p * L0:(p + 1) * L0], ob)
        assert sa == sb == 0
        assert np.array_equal(ya, yb), p
    assert [o.astuple() for o in oa] == [o.astuple() for o in ob]
    assert all(o.n_overflows > 0 for o in oa)
    if mixed:
        assert a.get_delay(OUT, 1) == L0 + 2 and a.get_delay(OUT, 2) == 0


# ---------------------------------------------------------------- 4. fractional values against float64

@pytest.mark.parametrize("rs,infmt,outfmt,sched,half,vin,vout", [
    (4, "S16_LE", "FLOAT_LE", SMALL, 31, (37, -25, 99), (-99, 12, -25)),
    (8, "FLOAT64_LE", "FLOAT64_LE", SMALL, 31, (37, -25, 99), (-99, 12, -25)),
    (8, "S24_LE", "FLOAT64_LE", BIG, 15, (-99, 99, 1), (37, -25, 50)),
    (4, "FLOAT_LE", "FLOAT_LE", BIG, 7, (37, -25, -1), (99, -99, 63)),
    (4, "S32_LE", "S16_LE", SMALL, 15, (37, None, -25), (None, 99, -99)),
    (8, "S16_LE", "S24_LE", SMALL, 7, (37, -25, 99), (-99, None, 12)),
    (8, "FLOAT64_LE", "S32_LE", BIG, 31, (None, -99, 50), (37, -25, 99))])
def test_fractional_values_against_the_float64_model(hip, rs, infmt, outfmt, sched, half, vin, vout):
    n_ch, periods, L0 = 3, 40, sched[0][0]
    nu, f0, _ = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    nu.enable_subdelay(half)
    for io, vals in ((IN, vin), (OUT, vout)):
        for ch, v in enumerate(vals):
            if v is not None:
                nu.set_subdelay(io, ch, v)
    nu.finalize()
    x = _raw(np.random.default_rng(half + rs), infmt, periods * L0, n_ch)
    got, sts = _run(nu, x, L0, periods)
    assert not any(sts)
    want = _model(hip, x, infmt, outfmt, n_ch, rs, L0, periods, half, f0,
                  [_const(v, periods) for v in vin], [_const(v, periods) for v in vout])
    _check(got, want, outfmt, n_ch, periods * L0, rs)
    assert [nu.get_subdelay(IN, ch) for ch in range(n_ch)] == [UNDEF if v is None else v for v in vin]


# ---------------------------------------------------------------- 5. run-time changes

@pytest.mark.parametrize("rs,infmt,outfmt", [(4, "FLOAT_LE", "FLOAT_LE"), (8, "FLOAT64_LE", "FLOAT64_LE"),
                                             (8, "S24_LE", "S16_LE")])
def test_run_time_changes_switch_the_taps_at_the_period(hip, rs, infmt, outfmt):
    """set_subdelay between block calls on inputs and outputs.  In SMALL the 512-frame segment is
    due in the periods b with (b + 1) % 8 == 0: changes land in such a period (15, 23), one period
    before one (14, 30) and elsewhere.  Every segment, however late it runs, must see the input
    filtered with the value that was in force in each frame's own period."""
    n_ch, periods, L0, half = 2, 48, 64, 31
    nu, f0, _ = _nupc(hip, rs, n_ch, infmt, outfmt, SMALL)
    nu.enable_subdelay(half)
    vin = [[37] * periods, [-25] * periods]
    vout = [[0] * periods, [99] * periods]
    for ch in range(n_ch):
        nu.set_subdelay(IN, ch, vin[ch][0])
        nu.set_subdelay(OUT, ch, vout[ch][0])
    nu.finalize()
    plan = {6: [(IN, 0, -60)], 14: [(IN, 1, 80)], 15: [(IN, 0, 45), (OUT, 0, -70)], 23: [(OUT, 1, -90), (IN, 1, 0)],
            30: [(IN, 0, 99), (IN, 1, -99)], 33: [(OUT, 0, 50)], 34: [(OUT, 0, 51)]}
    events = {}
    for p, chg in plan.items():
        for io, ch, v in chg:
            (vin if io == IN else vout)[ch][p:] = [v] * (periods - p)
        events[p] = lambda chg=chg: [nu.set_subdelay(io, ch, v) for io, ch, v in chg]
    x = _raw(np.random.default_rng(40 + rs), infmt, periods * L0, n_ch)
    got, sts = _run(nu, x, L0, periods, events)
    assert not any(sts)
    want = _model(hip, x, infmt, outfmt, n_ch, rs, L0, periods, half, f0, vin, vout)
    _check(got, want, outfmt, n_ch, periods * L0, rs)
    assert (nu.get_subdelay(IN, 0), nu.get_subdelay(IN, 1)) == (99, -99)
    assert (nu.get_subdelay(OUT, 0), nu.get_subdelay(OUT, 1)) == (51, -90)


# ---------------------------------------------------------------- 6. beside the other run-time controls

@pytest.mark.parametrize("rs,sched,half", [(4, SMALL, 31), (8, SMALL, 15), (8, BIG, 31)])
def test_with_mute_gain_and_a_coefficient_switch(hip, rs, sched, half):
    """an input mute that comes and goes (its zeros enter the filter's history), an output gain
    change, and a coefficient switch with the default one-block cross-fade: the output FIR runs on
    the blended, gained value"""
    n_ch, periods, L0 = 2, 48, sched[0][0]
    fmt = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    nu, f0, f1 = _nupc(hip, rs, n_ch, fmt, fmt, sched, sets=True)
    nu.enable_subdelay(half)
    vin, vout = (37, -25), (-60, 99)
    for ch in range(n_ch):
        nu.set_subdelay(IN, ch, vin[ch])
        nu.set_subdelay(OUT, ch, vout[ch])
    nu.finalize()
    n = periods * L0
    mute = np.zeros((n, n_ch), bool)
    mute[10 * L0:24 * L0, 0] = True
    gain = np.ones((n, n_ch))
    gain[20 * L0:, 1] = 0.5
    events = {10: lambda: nu.set_mute(IN, 0, 1), 24: lambda: nu.set_mute(IN, 0, 0),
              20: lambda: nu.set_output_gain(1, 0.5),
              30: lambda: [nu.set_coeff(f, 1) for f in range(2 * n_ch)]}
    x = _raw(np.random.default_rng(60 + rs), fmt, n, n_ch)
    got, sts = _run(nu, x, L0, periods, events)
    assert not any(sts)
    t_sw = nu.switch_frame()
    assert 30 * L0 <= t_sw < n - 2 * L0
    want = _model(hip, x, fmt, fmt, n_ch, rs, L0, periods, half, f0, [_const(v, periods) for v in vin],
                  [_const(v, periods) for v in vout], in_mute=mute, gain=gain, blend=(f1, t_sw, L0))
    _check(got, want, fmt, n_ch, n, rs)


def test_dither_on_a_filtered_s16_output(hip):
    """HP-TPDF dither behind the FIR, float64: tests/test_gpu_nupc_dither.py's bar for S16_LE at
    this realsize (equal but for rounding ties: no sample off by more than 1, at most 12 off)"""
    n_ch, periods, L0, half, rs = 2, 48, 64, 31, 8
    nu, f0, _ = _nupc(hip, rs, n_ch, "FLOAT64_LE", "S16_LE", SMALL, dither=[0, 1])
    nu.enable_subdelay(half)
    nu.set_subdelay(OUT, 0, 37)
    nu.set_subdelay(OUT, 1, -25)
    nu.finalize()
    x = _raw(np.random.default_rng(71), "FLOAT64_LE", periods * L0, n_ch)
    got, sts = _run(nu, x, L0, periods, {20: lambda: nu.set_subdelay(OUT, 1, 80)})
    assert not any(sts)
    want = _model(hip, x, "FLOAT64_LE", "S16_LE", n_ch, rs, L0, periods, half, f0, [None, None],
                  [[37] * periods, [-25] * 20 + [80] * (periods - 20)], dither=(0, 1))
    fm = _fmts("S16_LE", n_ch)
    d = np.abs(nr.ints(got, fm, periods * L0) - nr.ints(want, fm, periods * L0))
    print("max count difference %d, samples off %d" % (d.max(), (d > 0).sum()))
    assert d.max() <= 1, d.max()
    assert (d > 0).sum() <= 12, (d > 0).sum()


# ---------------------------------------------------------------- 7. unchanged when unused

@pytest.mark.parametrize("rs,infmt,outfmt", [(4, "S24_LE", "S16_LE"), (8, "FLOAT64_LE", "S24_LE")])
def test_enabled_without_a_filter_changes_nothing(hip, rs, infmt, outfmt):
    n_ch, periods, L0 = 3, 24, 64
    a, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, gain=4.0)
    b, _, _ = _nupc(hip, rs, n_ch, infmt, outfmt, gain=4.0)
    a.enable_subdelay(31)
    a.set_subdelay(IN, 1, UNDEF)
    a.finalize()
    b.finalize()
    oa, ob = _ovf(outfmt, n_ch, hip), _ovf(outfmt, n_ch, hip)
    x = _raw(np.random.default_rng(29), infmt, periods * L0, n_ch, 0.3)
    ya, sa = _run(a, x, L0, periods, ovf=oa)
    yb, sb = _run(b, x, L0, periods, ovf=ob)
    assert sa == sb and np.array_equal(ya, yb)
    assert [o.astuple() for o in oa] == [o.astuple() for o in ob]
    assert a.get_subdelay(IN, 1) == UNDEF and a.get_delay(IN, 1) == 0


@pytest.mark.parametrize("rs", [4, 8])
def test_filters_on_the_outputs_only_leave_the_input_path_alone(hip, rs):
    """outputs filtered, inputs not: the plain convolver's float output through the model FIR"""
    n_ch, periods, L0, half = 2, 40, 64, 15
    fmt = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    a, _, _ = _nupc(hip, rs, n_ch, "S24_LE", fmt)
    b, _, _ = _nupc(hip, rs, n_ch, "S24_LE", fmt)
    a.enable_subdelay(half)
    a.set_subdelay(OUT, 0, 37)
    a.set_subdelay(OUT, 1, -25)
    a.finalize()
    b.finalize()
    x = _raw(np.random.default_rng(31), "S24_LE", periods * L0, n_ch)
    ya, sa = _run(a, x, L0, periods)
    yb, sb = _run(b, x, L0, periods)
    assert not any(sa) and not any(sb)
    fm = _fmts(fmt, n_ch)
    plain = nr.decode(yb, fm, periods * L0)
    want = np.stack([_fir(plain[:, c], [v] * periods, half, rs, L0) for c, v in enumerate((37, -25))], axis=1)
    got = nr.decode(ya, fm, periods * L0)
    for c in range(n_ch):
        err = cases.rel_rms(got[:, c], want[:, c])
        print("rel rms ch %d: %.3g" % (c, err))
        assert err <= (1e-5 if rs == 4 else 1e-12), (c, err)


# ---------------------------------------------------------------- 8. misuse

def test_misuse_returns_the_stated_codes_and_changes_nothing(hip):
    n_ch, L0, half = 2, 64, 15
    L = hip.lib()
    a, _, _ = _nupc(hip, 4, n_ch, "S16_LE", "S16_LE")
    b, _, _ = _nupc(hip, 4, n_ch, "S16_LE", "S16_LE")
    for half_bad, msg in ((0, b"Invalid half filter length 0."), (32, b"The filter_length must be at least 2 x sdf_length + 1."),
                          (512, b"The filter_length must be at least 2 x sdf_length + 1.")):
        assert L.bfhip_nupc_enable_subdelay(a.h, half_bad, 9.0) == EINVAL
        assert L.bfhip_nupc_last_error() == msg
    d, _, _ = _nupc(hip, 4, 1, "S16_LE", "S16_LE", ([2048], [1]))
    assert L.bfhip_nupc_enable_subdelay(d.h, 512, 9.0) == EINVAL          # filter block size above the limit
    assert b"not supported" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_enable_subdelay(d.h, 40, 9.0) == 0
    d.close()
    assert L.bfhip_nupc_set_subdelay(a.h, IN, 0, 100) == EINVAL          # before finalize too
    assert L.bfhip_nupc_set_subdelay(a.h, 2, 0, 10) == EINVAL
    assert L.bfhip_nupc_set_subdelay(a.h, IN, n_ch, 10) == EINVAL
    assert a.get_subdelay(IN, 0) == UNDEF
    for nu in (a, b):
        nu.enable_subdelay(half, 4.5)                                     # beta is accepted and ignored
        nu.set_subdelay(IN, 0, 37)
        nu.set_subdelay(OUT, 1, -25)
        nu.finalize()
    assert a.get_subdelay(IN, 0) == 37 and a.get_subdelay(OUT, 1) == -25
    x = _raw(np.random.default_rng(83), "S16_LE", 12 * L0, n_ch)
    for p in range(12):
        if p == 4:
            assert L.bfhip_nupc_set_subdelay(a.h, IN, 1, 10) == EINVAL    # no filter on this channel
            assert L.bfhip_nupc_set_subdelay(a.h, OUT, 0, 0) == EINVAL
            assert L.bfhip_nupc_set_subdelay(a.h, IN, 0, 100) == EINVAL
            assert L.bfhip_nupc_set_subdelay(a.h, IN, 0, -100) == EINVAL
            assert L.bfhip_nupc_set_subdelay(a.h, OUT, 1, 100) == EINVAL
            assert L.bfhip_nupc_enable_subdelay(a.h, 7, 9.0) == ESTATE
            assert L.bfhip_nupc_get_subdelay(a.h, IN, n_ch) == EINVAL
            assert (a.get_subdelay(IN, 0), a.get_subdelay(IN, 1), a.get_subdelay(OUT, 1)) == (37, UNDEF, -25)
        if p == 8:
            for nu in (a, b):
                nu.set_subdelay(IN, 0, -80)
            assert a.get_subdelay(IN, 0) == -80
        sa, ya = a.block(x[p * L0:(p + 1) * L0])
        sb, yb = b.block(x[p * L0:(p + 1) * L0])
        assert sa == sb == 0 and np.array_equal(ya, yb), p
    c, _, _ = _nupc(hip, 4, n_ch, "S16_LE", "S16_LE")
    c.set_subdelay(OUT, 0, 10)                                            # a filter without enable_subdelay
    assert L.bfhip_nupc_finalize(c.h) == EINVAL
    assert b"enable_subdelay" in L.bfhip_nupc_last_error()


# ---------------------------------------------------------------- allocation faults

def test_every_allocation_failure_of_a_sub_delayed_convolver_is_an_error_code(hip):
    """bfhip_selftest_fail_alloc walked over a sub-delayed convolver's life, the way
    tests/test_gpu_alloc_faults.py walks the plain one's: the n-th device / pinned allocation
    fails, n = 1, 2, ... until a life no longer reaches it.  Every failure is a BfhipError, destroy
    cleans up, and a clean life works afterwards."""
    L = hip.lib()
    rng = np.random.default_rng(5)
    h = (rng.standard_normal(500) / 40).astype(np.float32)
    xs = _raw(rng, "S16_LE", 64, 2)

    def life():
        nu = None
        try:
            nu = hip.Nupc([64, 128], [2, 2], 4, 2, 2)
            nu.set_interleaved(0, "S16_LE")
            nu.set_interleaved(1, "S16_LE")
            nu.enable_dither([1], 300)
            nu.enable_subdelay(31)
            nu.set_subdelay(IN, 0, 37)
            nu.set_subdelay(OUT, 1, -25)
            nu.set_maxdelay(IN, 1, 100)
            nu.add_filter(0, 0, h)
            nu.add_filter(1, 1, h)
            nu.finalize()
            out = [nu.block(xs)[1] for _ in range(3)]
        finally:
            left = L.bfhip_selftest_fail_alloc(0)
            if nu is not None:
                nu.close()
        return left, np.concatenate(out)

    _, clean = life()
    errors, absorbed, n = 0, 0, 0
    while True:
        n += 1
        assert n < 400
        L.bfhip_selftest_fail_alloc(n)
        try:
            left, _ = life()
            if left > 0:
                break                                     # a whole life makes n - left allocations
            absorbed += 1
        except hip.BfhipError:
            errors += 1
    print("allocations walked %d, errors %d, absorbed %d" % (n - 1, errors, absorbed))
    assert n - 1 >= 30 and errors >= n - 1 - 6
    _, again = life()
    assert np.array_equal(again, clean)
