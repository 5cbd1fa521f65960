"""GPU: per-channel integer delay and mute on the raw I/O blocks of the non-uniform convolver
(bfhip_nupc_set_maxdelay / _set_delay / _set_mute / _get_delay, include/bfhip_nupc.h).  The
reference does these in dai.c on its raw period buffers (do_mute then update_delay on input,
update_delay then mute on output); with a period of L0 frames the nupc must produce exactly that.
The model is the oracle's integer delay (bfo_delay_new / bfo_delay_update, pinned to delay.c by
tests/test_oracle_delay.py), applied per raw channel with fragment L0: the delayed, muted nupc
equals a plain nupc fed the model's input, with the model applied to its output, byte for byte."""
import numpy as np
import pytest

import bforacle as bo
from nupc_chain_ref import Model

pytestmark = pytest.mark.gpu
SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])               # offsets 0, 128, 384, 896; 3968 taps
C4 = ([64, 128, 256, 512, 1024, 2048], [2, 2, 2, 2, 2, 4])  # configs[4]-shaped, 12160 taps
L0 = 64
IN, OUT = 0, 1
EINVAL, ESTATE = -1, -5


def _raw(rng, fmt, frames, n_ch, amp=0.3):
    nbytes, sbytes, isfloat, _ = bo.SAMPLE_FORMATS[fmt]
    x = rng.standard_normal((frames, n_ch)) * amp
    if isfloat:
        return x.astype(np.float32 if nbytes == 4 else np.float64).view(np.uint8).reshape(frames, -1)
    full = 1 << (8 * sbytes - 1)
    v = np.clip(np.round(x * full), -full, full - 1).astype("<i8")
    return np.ascontiguousarray(v.view(np.uint8).reshape(frames, n_ch, 8)[:, :, :nbytes]).reshape(frames, -1)


def _nupc(hip, rs, n_ch, infmt, outfmt, sched=SMALL, seed=7, dither=None, sets=False, gain=1.0):
    nu = hip.Nupc(sched[0], sched[1], rs, n_ch, n_ch)
    nu.set_interleaved(0, infmt)
    nu.set_interleaved(1, outfmt)
    if dither:
        nu.enable_dither(dither, 300)
    rng = np.random.default_rng(seed)
    n = min(nu.taps, 3000)
    env = np.exp(-np.arange(n) / 400.0)
    taps = []
    for o in range(n_ch):
        for i in (o, (o + 1) % n_ch):
            h = rng.standard_normal(n) * env * gain / 12.0
            nu.add_filter(i, o, h)
            taps.append(h)
    if sets:
        for f, h in enumerate(taps):
            nu.add_coeff(f, -0.5 * h[::-1].copy())
    return nu


def _ovf(outfmt, n_ch, hip):
    nbytes, sbytes, isfloat, _ = bo.SAMPLE_FORMATS[outfmt]
    mx = 1.0 if isfloat else float((1 << (8 * sbytes - 1)) - 1)
    return (hip.Overflow * n_ch)(*[hip.Overflow(0, 0, 0.0, mx) for _ in range(n_ch)])


def _configure(nu, io, spec):
    for ch, (d, m) in enumerate(spec):
        nu.set_maxdelay(io, ch, m)
        nu.set_delay(io, ch, d)


# ---------------------------------------------------------------- 1. input delay and mute

@pytest.mark.parametrize("rs,infmt,sched,n_ch,periods", [
    (4, "S16_LE", SMALL, 3, 40), (4, "S24_LE", SMALL, 3, 40), (4, "S32_LE", SMALL, 3, 40),
    (4, "FLOAT_LE", SMALL, 3, 40), (4, "FLOAT64_LE", SMALL, 3, 40),
    (8, "S24_LE", SMALL, 3, 40), (8, "FLOAT64_LE", SMALL, 3, 40), (8, "S16_LE", SMALL, 3, 40),
    (8, "FLOAT64_LE", C4, 2, 100), (4, "S24_LE", C4, 2, 100)])
def test_input_delay_and_mute_equal_the_model_on_the_input(hip, rs, infmt, sched, n_ch, periods):
    """delays below L0, equal to L0 and several fragments long (fixed and changeable), a mute that
    comes and goes and a run-time change: the convolver with them gives the bytes of a plain one
    fed the model's delayed, muted input"""
    outfmt = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    spec = [(L0 - 5, -1), (L0, -1), (3 * L0 + 7, 4 * L0)][:n_ch]
    if n_ch == 2:
        spec = [(L0, -1), (3 * L0 + 7, 4 * L0)]
    a = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    b = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    _configure(a, IN, spec)
    a.finalize()
    b.finalize()
    m = Model(IN, infmt, spec, L0)
    x = _raw(np.random.default_rng(rs * 100 + len(infmt)), infmt, periods * L0, n_ch)
    for p in range(periods):
        if p == 10:
            a.set_mute(IN, 0, 1); m.lines[0].muted = True
        if p == 25:
            a.set_mute(IN, 0, 0); m.lines[0].muted = False
        if p == 20:
            a.set_delay(IN, n_ch - 1, 2 * L0 + 1); m.lines[-1].req = 2 * L0 + 1
        if p == 31:
            a.set_delay(IN, n_ch - 1, 4 * L0); m.lines[-1].req = 4 * L0
        xb = x[p * L0:(p + 1) * L0]
        sa, ya = a.block(xb)
        sb, yb = b.block(m.run(xb))
        assert sa == sb == 0
        assert np.array_equal(ya, yb), p
        for ch in range(n_ch):
            assert a.get_delay(IN, ch) == m.lines[ch].cur


# ---------------------------------------------------------------- 2. output delay and mute (+ 5. overflow)

@pytest.mark.parametrize("rs,outfmt,dither", [
    (4, "S16_LE", [0, 2]), (8, "S24_LE", None), (4, "S24_4LE", [1]), (8, "S32_LE", [0, 1, 2]),
    (4, "FLOAT_LE", None), (8, "FLOAT64_LE", None), (8, "S24_LE", [2])])
def test_output_delay_and_mute_equal_the_model_on_the_output(hip, rs, outfmt, dither):
    """the model applied to a plain convolver's output bytes, with dither, output gain and a
    coefficient switch with cross-fade in flight; the status bits and overflow structs are the
    plain run's (some samples clip): they count the undelayed, unmuted samples"""
    n_ch = 3
    infmt = "FLOAT_LE" if rs == 4 else "FLOAT64_LE"
    spec = [(L0 - 1, -1), (L0, 3 * L0), (2 * L0 + 5, -1)]
    a = _nupc(hip, rs, n_ch, infmt, outfmt, dither=dither, sets=True, gain=6.0)
    b = _nupc(hip, rs, n_ch, infmt, outfmt, dither=dither, sets=True, gain=6.0)
    _configure(a, OUT, spec)
    a.finalize()
    b.finalize()
    m = Model(OUT, outfmt, spec, L0)
    oa, ob = _ovf(outfmt, n_ch, hip), _ovf(outfmt, n_ch, hip)
    x = _raw(np.random.default_rng(17 + rs), infmt, 60 * L0, n_ch)
    clipped = 0
    for p in range(60):
        if p == 5:
            for nu in (a, b):
                nu.set_output_gain(0, 0.5)
        if p == 12:
            for nu in (a, b):
                nu.set_crossfade(150)
                for f in range(2 * n_ch):
                    nu.set_coeff(f, 1)
        if p == 8:
            a.set_mute(OUT, 2, 1); m.lines[2].muted = True
        if p == 30:
            a.set_mute(OUT, 2, 0); m.lines[2].muted = False
        if p == 14:
            a.set_delay(OUT, 1, 3 * L0); m.lines[1].req = 3 * L0       # increase, during the fade
        if p == 33:
            a.set_delay(OUT, 1, 10); m.lines[1].req = 10               # decrease across L0
        if p == 40:
            a.set_mute(OUT, 0, 1); m.lines[0].muted = True
        xb = x[p * L0:(p + 1) * L0]
        sa, ya = a.block(xb, oa)
        sb, yb = b.block(xb, ob)
        assert sa == sb
        assert np.array_equal(ya, m.run(yb)), p
        assert [o.astuple() for o in oa] == [o.astuple() for o in ob], p
        clipped = sum(o.n_overflows for o in ob)
        for ch in range(n_ch):
            assert a.get_delay(OUT, ch) == m.lines[ch].cur
    assert a.switch_frame() == b.switch_frame() >= 0
    if not bo.SAMPLE_FORMATS[outfmt][2]:
        assert clipped > 0


# ---------------------------------------------------------------- 3. run-time sequences

def _random_run(hip, rs, infmt, outfmt, seed, periods, sched=SMALL):
    n_ch = 3
    spec_in = [(10, 3 * L0 + 10), (20, -1), (L0, L0)]
    spec_out = [(0, 5 * L0), (2 * L0 - 3, 2 * L0 - 3), (70, -1)]
    a = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    b = _nupc(hip, rs, n_ch, infmt, outfmt, sched)
    _configure(a, IN, spec_in)
    _configure(a, OUT, spec_out)
    a.finalize()
    b.finalize()
    L = hip.lib()
    assert L.bfhip_nupc_set_maxdelay(a.h, IN, 0, 100) == ESTATE
    assert L.bfhip_nupc_set_maxdelay(a.h, OUT, 2, 100) == ESTATE
    assert L.bfhip_nupc_set_delay(a.h, IN, 1, -1) == EINVAL
    assert L.bfhip_nupc_set_delay(a.h, OUT, 0, -5) == EINVAL
    assert L.bfhip_nupc_set_delay(a.h, OUT, n_ch, 5) == EINVAL
    assert L.bfhip_nupc_set_mute(a.h, 2, 0, 1) == EINVAL
    mi, mo = Model(IN, infmt, spec_in, L0), Model(OUT, outfmt, spec_out, L0)
    rng = np.random.default_rng(seed)
    x = _raw(rng, infmt, periods * L0, n_ch)
    choices = [0, 1, L0 - 1, L0, L0 + 1, 2 * L0 - 3, 2 * L0, 2 * L0 + 17, 3 * L0 + 10, 5 * L0, 5 * L0 + 1, 9 * L0]
    for p in range(periods):
        for io, nu_m in ((IN, mi), (OUT, mo)):
            for ch in range(n_ch):
                if rng.random() < 0.2:
                    d = int(rng.choice(choices)) if rng.random() < 0.8 else int(rng.integers(0, 6 * L0))
                    a.set_delay(io, ch, d)
                    nu_m.lines[ch].req = d
                if rng.random() < 0.08:
                    nu_m.lines[ch].muted = not nu_m.lines[ch].muted
                    a.set_mute(io, ch, nu_m.lines[ch].muted)
        xb = x[p * L0:(p + 1) * L0]
        sa, ya = a.block(xb)
        sb, yb = b.block(mi.run(xb))
        assert sa == sb == 0
        assert np.array_equal(ya, mo.run(yb)), p
        for io, nu_m in ((IN, mi), (OUT, mo)):
            for ch in range(n_ch):
                assert a.get_delay(io, ch) == nu_m.lines[ch].cur, (p, io, ch)
    # the fixed channels never moved
    assert a.get_delay(IN, 1) == 20 and a.get_delay(OUT, 2) == 70
    return mi, mo


@pytest.mark.parametrize("rs,infmt,outfmt,seed", [
    (4, "S16_LE", "S32_LE", 1), (4, "S24_LE", "S24_LE", 2), (8, "FLOAT64_LE", "FLOAT64_LE", 3),
    (8, "S32_LE", "S16_LE", 4)])
def test_random_delay_changes_and_mute_toggles(hip, rs, infmt, outfmt, seed):
    """seeded per-period changes on both sides across the <= L0 / > L0 boundary, values above
    maxdelay (ignored), a fixed channel (ignores changes), get_delay == curdelay every period,
    EINVAL for delay < 0, ESTATE for set_maxdelay after finalize"""
    mi, mo = _random_run(hip, rs, infmt, outfmt, seed, 150)
    # the sequences did move the changeable lines
    assert mi.lines[0].cur != 10 or mo.lines[0].cur != 0


def test_random_changes_configs4_shape(hip):
    _random_run(hip, 8, "FLOAT64_LE", "S24_4LE", 11, 100, sched=C4)


# ---------------------------------------------------------------- 4. async equals sync

def test_block_dev_eight_in_flight_equals_block(hip):
    """block_dev with 8 periods handed in before one sync, delays and mutes changed between the
    calls, gives the bytes of the synchronous block() run"""
    import torch
    n_ch, rs, infmt, outfmt, periods = 2, 4, "S16_LE", "S32_LE", 64
    spec_in = [(L0 + 3, 4 * L0), (5, L0)]
    spec_out = [(2 * L0, 3 * L0), (0, L0 + 1)]
    rng = np.random.default_rng(23)
    x = _raw(rng, infmt, periods * L0, n_ch)
    plan = []
    for p in range(periods):
        ev = []
        for io in (IN, OUT):
            for ch in range(n_ch):
                if rng.random() < 0.25:
                    ev.append(("d", io, ch, int(rng.integers(0, 5 * L0))))
                if rng.random() < 0.1:
                    ev.append(("m", io, ch, int(rng.integers(0, 2))))
        plan.append(ev)

    def make():
        nu = _nupc(hip, rs, n_ch, infmt, outfmt, seed=3)
        _configure(nu, IN, spec_in)
        _configure(nu, OUT, spec_out)
        nu.finalize()
        return nu

    def apply(nu, p):
        for kind, io, ch, v in plan[p]:
            (nu.set_delay if kind == "d" else nu.set_mute)(io, ch, v)

    a = make()
    want = []
    for p in range(periods):
        apply(a, p)
        st, y = a.block(x[p * L0:(p + 1) * L0])
        assert st == 0
        want.append(y)
    b = make()
    ib, ob = x.shape[1] * L0, b.out_bytes
    din = torch.empty(8 * ib, dtype=torch.uint8, device="cuda")
    dout = torch.zeros(8 * ob, dtype=torch.uint8, device="cuda")
    got = []
    for g in range(0, periods, 8):
        din.copy_(torch.from_numpy(np.ascontiguousarray(x[g * L0:(g + 8) * L0]).ravel()))
        torch.cuda.synchronize()
        for i in range(8):
            apply(b, g + i)
            b.block_dev(din[i * ib:(i + 1) * ib], dout[i * ob:(i + 1) * ob])
        assert b.sync() == 0
        y = dout.cpu().numpy()
        got += [y[i * ob:(i + 1) * ob].copy() for i in range(8)]
    for p in range(periods):
        assert np.array_equal(got[p], want[p]), p


# ---------------------------------------------------------------- 6. unused means unchanged

@pytest.mark.parametrize("rs,infmt,outfmt", [(4, "S24_LE", "S16_LE"), (8, "FLOAT64_LE", "S24_4LE")])
def test_maxdelay_with_zero_delays_changes_nothing(hip, rs, infmt, outfmt):
    """maxdelay set on every channel, all delays 0 (also re-requested at run time), nothing muted:
    the bytes and overflow structs of a plain convolver"""
    n_ch = 3
    a = _nupc(hip, rs, n_ch, infmt, outfmt, gain=4.0)
    b = _nupc(hip, rs, n_ch, infmt, outfmt, gain=4.0)
    for io in (IN, OUT):
        for ch in range(n_ch):
            a.set_maxdelay(io, ch, 1000 + 64 * ch)
    a.finalize()
    b.finalize()
    oa, ob = _ovf(outfmt, n_ch, hip), _ovf(outfmt, n_ch, hip)
    x = _raw(np.random.default_rng(29), infmt, 30 * L0, n_ch)
    for p in range(30):
        if p == 7:
            for io in (IN, OUT):
                a.set_delay(io, 1, 0)
                a.set_mute(io, 2, 0)
        sa, ya = a.block(x[p * L0:(p + 1) * L0], oa)
        sb, yb = b.block(x[p * L0:(p + 1) * L0], ob)
        assert sa == sb and np.array_equal(ya, yb), p
        assert [o.astuple() for o in oa] == [o.astuple() for o in ob]
    for io in (IN, OUT):
        for ch in range(n_ch):
            assert a.get_delay(io, ch) == 0
