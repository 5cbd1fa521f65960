"""GPU: equaliser curves rendered on the device with minimum phase (bfhip_nupc_reserve_eq_minimum /
_render_eq_mode_async / _render_eq_mode, include/bfhip_nupc.h).

What must hold: the minimum-mode render alone is the float64 model's (tests/eq_minphase_ref.py) at
the project's parity bars, float32 1e-5 / float64 1e-12 relative RMS, at the smallest two lengths,
with a skipped band, at the largest one-workgroup length (R = 16384) and on the big-FFT sequence with
one combine pass of radix 2, 4, 8 and with two passes; a render is a pure function of its arguments;
linear mode through the new calls has the bytes of bfhip_nupc_render_eq; a minimum render into an
idle set followed by a switch has the BYTES of update_coeff_async with the array the synchronous
minimum render returned, and the output after the switch is the float64 model's (tests/nupc_ref.py);
a flat curve passes the input through with no R/2 frames of delay, where the linear render delays it
by R/2; the reservation alone, and a minimum render into an idle set before the switch, change no
output byte; and every argument and state error answers its code and changes nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import eq_minphase_ref
import eq_ref
import nupc_ref

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
DT = {4: np.float32, 8: np.float64}
EINVAL, ESTATE = -1, -5
LINEAR, MINIMUM = 0, 1
# the four curves of tests/test_gpu_nupc_eq.py (all magnitudes above 0) and one of +-40 dB
CURVES = {"flat": eq_ref.flat(), "130 bands": eq_ref.random_bands(130, 7), "knot on a bin": eq_ref.knot_on_a_bin(),
          "skipped band": eq_ref.skipped_band(), "130 bands, 40 dB": eq_ref.random_bands(130, 3, db=40.0)}
LENGTHS = [8, 16, 64, 16384, 32768, 65536, 131072, 262144]
# schedule, blocks run, block the render starts before, block the switch is requested before, render length
SMALL = dict(sched=([16, 32, 64], [2, 2, 4]), n_blocks=60, b_render=3, b_switch=12, R=256)
BIG = dict(sched=([64, 256, 1024, 4096, 16384], [4, 4, 4, 4, 1]), n_blocks=1300, b_render=3, b_switch=40, R=32768)


def _noise(seed, n, dt):
    return (np.random.default_rng(seed).standard_normal(n) / np.sqrt(n)).astype(dt)


@functools.lru_cache(maxsize=None)
def _model(R, name, mode=MINIMUM):
    taps = (eq_minphase_ref if mode == MINIMUM else eq_ref).render(R, *CURVES[name])
    taps.setflags(write=False)
    return taps


_renderers = {}


def _make_renderer(hip, rs, minimum=True):
    """a single 16384-frame segment, 1 048 576 taps in float32 and 262 144 in float64, one filter with
    a second set to render into"""
    nu = hip.Nupc([16384], [64 if rs == 4 else 16], rs, 1, 1)
    nu.reserve_update()
    nu.reserve_eq(nu.taps)
    if minimum:
        nu.reserve_eq_minimum()
    nu.add_filter(0, 0, _noise(1, 64, DT[rs]))
    assert nu.add_coeff(0, _noise(2, 64, DT[rs])) == 1
    nu.finalize()
    return nu


def _renderer(hip, rs):
    """one convolver per precision, shared by the tests that only make synchronous renders on it"""
    if rs not in _renderers:
        _renderers[rs] = _make_renderer(hip, rs)
    return _renderers[rs]


def _old_render_eq(hip, nu, R, curve):
    """bfhip_nupc_render_eq itself, the call without a mode"""
    out = np.zeros(R, nu.dt)
    f, m, p = (hip._darr(list(v)) for v in curve)
    assert hip.lib().bfhip_nupc_render_eq(nu.h, R, len(curve[0]), f, m, p, out.ctypes.data_as(C.c_void_p)) == 0
    return out


# ---------------------------------------------------------------- 1: the render alone

@pytest.mark.parametrize("R", LENGTHS)
@pytest.mark.parametrize("rs", [4, 8])
def test_minimum_render_is_the_float64_model(hip, rs, R):
    nu = _renderer(hip, rs)
    for name, curve in CURVES.items():
        got = nu.render_eq(R, *curve, mode="minimum")
        assert got.dtype == DT[rs] and got.shape == (R,)
        err = cases.rel_rms(got, _model(R, name))
        print("rs %d R %d %s: rel rms %.3g (limit %g)" % (rs, R, name, err, TOL[rs]))
        assert err <= TOL[rs], name
        assert np.array_equal(got, nu.render_eq(R, *curve, mode="minimum")), name       # a pure function of its arguments


def test_minimum_render_of_the_full_room_correction_length(hip):
    nu, R = _renderer(hip, 4), 1048576
    for name in ("130 bands", "130 bands, 40 dB"):
        got = nu.render_eq(R, *CURVES[name], mode="minimum")
        err = cases.rel_rms(got, _model(R, name))
        print("rs 4 R %d %s: rel rms %.3g (limit %g)" % (R, name, err, TOL[4]))
        assert err <= TOL[4], name
        assert np.array_equal(got, nu.render_eq(R, *CURVES[name], mode="minimum")), name


@pytest.mark.parametrize("R", [64, 32768])
@pytest.mark.parametrize("rs", [4, 8])
def test_linear_mode_has_the_bytes_of_render_eq(hip, rs, R):
    nu = _renderer(hip, rs)
    for name, curve in CURVES.items():
        want = _old_render_eq(hip, nu, R, curve)
        assert np.any(want)
        assert np.array_equal(nu.render_eq(R, *curve, mode="linear"), want), name
        assert np.array_equal(nu.render_eq(R, *curve, mode=hip.EQ_LINEAR), want), name
        assert np.array_equal(nu.render_eq(R, *curve), want), name
        assert not np.array_equal(nu.render_eq(R, *curve, mode="minimum"), want), name


# ---------------------------------------------------------------- runs with a switch onto a rendered set

class Run:
    """one filter with two sets of flat noise; `how` rewrites set 1 before block b_render:
    "eq" render_eq_async in `mode`, "upload" update_coeff_async with the array render_eq returns in
    `mode`, None not at all; the switch 0 -> 1 is requested before block b_switch"""

    def __init__(self, hip, rs, plan, out_fmt, how, mode="minimum", reserve_min=True, wait_at_switch=False,
                 curve="130 bands", switch=True):
        dt = DT[rs]
        self.nu = nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, 1, 1)
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, out_fmt)
        nu.reserve_update()
        nu.reserve_eq(plan["R"])
        if reserve_min:
            nu.reserve_eq_minimum()
        self.h = [_noise(11, nu.taps, dt), _noise(12, nu.taps, dt)]
        nu.add_filter(0, 0, self.h[0])
        assert nu.add_coeff(0, self.h[1]) == 1
        nu.finalize()
        self.L0, R = nu.L0, plan["R"]
        self.x = (np.random.default_rng(5).standard_normal((plan["n_blocks"] * nu.L0, 1)) * 0.02).astype(dt)
        got = []
        for b in range(plan["n_blocks"]):
            if b == plan["b_render"] and how == "eq":
                nu.render_eq_async(0, 1, R, *CURVES[curve], mode=mode)
                if not wait_at_switch:
                    assert nu.update_wait() == 0
            if b == plan["b_render"] and how == "upload":
                nu.update_coeff_async(0, 1, nu.render_eq(R, *CURVES[curve], mode=mode))
                assert nu.update_wait() == 0
            if b == plan["b_switch"] and switch:
                if how == "eq" and wait_at_switch:
                    assert nu.update_wait() == 0
                nu.set_coeff(0, 1)
            got.append(nu.block(self.x[b * nu.L0:(b + 1) * nu.L0]))
        self.status = [s for s, _ in got]
        self.raw = np.concatenate([r for _, r in got])
        self.t_sw = nu.switch_frame()


# ---------------------------------------------------------------- 2: same bits as the upload path

@pytest.mark.parametrize("rs,plan,out_fmt", [(4, SMALL, "S24_4LE"), (8, BIG, "FLOAT64_LE")], ids=["f32 lds", "f64 big"])
def test_minimum_render_into_a_set_has_the_bits_of_the_upload(hip, rs, plan, out_fmt):
    a = Run(hip, rs, plan, out_fmt, "eq")
    b = Run(hip, rs, plan, out_fmt, "upload")
    assert a.nu.taps >= plan["R"] and a.t_sw == b.t_sw and a.t_sw > 0
    assert (a.t_sw + a.L0 + a.nu.taps) < len(a.x), "the run must go on beyond the switch window"
    assert a.status == b.status
    assert np.array_equal(a.raw, b.raw)
    assert np.any(a.raw[(a.t_sw + a.L0) * a.nu.out_bytes // a.L0:])


# ---------------------------------------------------------------- 3: against the float64 model end to end

@pytest.mark.parametrize("rs", [4, 8])
def test_output_after_the_switch_is_the_models(hip, rs):
    r = Run(hip, rs, SMALL, FF[rs], "eq")
    L0, n = r.L0, len(r.x)
    eq = np.concatenate([_model(SMALL["R"], "130 bands"), np.zeros(r.nu.taps - SMALL["R"])])
    x = r.x.astype(np.float64)
    ys = [nupc_ref.convolve(x, [(0, 0, h, 1.0, 1.0)], 1) for h in (r.h[0], eq)]
    want = nupc_ref.switched(ys, [(r.t_sw, L0, 1)])
    fmts = [nupc_ref.fmt(FF[rs])]
    want = nupc_ref.decode(nupc_ref.encode(want, fmts, L0)[0], fmts, n)
    got = nupc_ref.decode(r.raw, fmts, n)
    err = cases.rel_rms(got, want)
    print("rs %d: rel rms whole run %.3g (limit %g)" % (rs, err, TOL[rs]))
    assert err <= TOL[rs]
    for b in range(0, n, L0):
        if np.abs(want[b:b + L0]).max() > 0:
            assert cases.rel_rms(got[b:b + L0], want[b:b + L0]) <= TOL[rs], b // L0
    t = r.t_sw + L0                                # behind the fade: the rendered set alone
    assert t < n - L0 and cases.rel_rms(got[t:], ys[1][t:]) <= TOL[rs]


@pytest.mark.parametrize("rs", [4, 8])
def test_flat_curve_adds_no_delay_where_the_linear_render_adds_half_its_length(hip, rs):
    """the filter's scales are 1 and a flat curve of magnitude 1 is a unit pulse: behind the cross-fade
    the output is the input itself in minimum mode and the input R/2 frames earlier in linear mode"""
    R, fmts = SMALL["R"], [nupc_ref.fmt(FF[rs])]
    for mode, shift in (("minimum", 0), ("linear", R // 2)):
        r = Run(hip, rs, SMALL, FF[rs], "eq", mode=mode, curve="flat")
        n = len(r.x)
        got = nupc_ref.decode(r.raw, fmts, n)[:, 0]
        x = r.x.astype(np.float64)[:, 0]
        t = r.t_sw + r.L0
        assert r.t_sw > 0 and t - shift > 0 and n - t >= 16 * r.L0
        err = cases.rel_rms(got[t:], x[t - shift:n - shift])
        other = cases.rel_rms(got[t:], x[t - (R // 2 - shift):n - (R // 2 - shift)])
        print("rs %d %s: rel rms against the input %d frames earlier %.3g (limit %g); against the other shift %.3g"
              % (rs, mode, shift, err, TOL[rs], other))
        assert err <= TOL[rs], mode
        assert other > 0.5, mode


# ---------------------------------------------------------------- 4: no side effects

def test_the_reservation_alone_changes_no_byte(hip):
    a = Run(hip, 4, SMALL, "S24_4LE", None, reserve_min=True)
    b = Run(hip, 4, SMALL, "S24_4LE", None, reserve_min=False)
    assert a.t_sw == b.t_sw and np.array_equal(a.raw, b.raw)
    a = Run(hip, 4, SMALL, "S24_4LE", "eq", mode="linear", reserve_min=True)     # and no byte of a linear render
    b = Run(hip, 4, SMALL, "S24_4LE", "eq", mode="linear", reserve_min=False)
    assert a.t_sw == b.t_sw and np.array_equal(a.raw, b.raw)


@pytest.mark.parametrize("rs,plan", [(4, SMALL), (8, BIG)], ids=["f32 lds", "f64 big"])
def test_minimum_render_into_an_idle_set_changes_no_byte_before_the_switch(hip, rs, plan):
    plan = dict(plan, n_blocks=plan["b_switch"] + 20)
    a = Run(hip, rs, plan, FF[rs], "eq", wait_at_switch=True, switch=False)     # rendered, never switched to
    b = Run(hip, rs, plan, FF[rs], None, switch=False)
    assert a.nu.update_wait() == 0
    assert np.array_equal(a.raw, b.raw)
    a = Run(hip, rs, plan, FF[rs], "eq", wait_at_switch=True)                   # the render beside the periods
    b = Run(hip, rs, plan, FF[rs], None)
    cut = a.t_sw // a.L0 * a.nu.out_bytes
    assert a.t_sw == b.t_sw and cut > 0 and np.array_equal(a.raw[:cut], b.raw[:cut])


def test_calls_while_a_minimum_render_is_in_flight(hip):
    """1 048 576 taps into 64 partitions of 16384: the host calls below take microseconds, the device
    work does not; that the rewrite was still in flight behind the last of them is asserted"""
    L = hip.lib()
    nu = _make_renderer(hip, 4)
    h, R = nu.h, nu.taps
    out = np.zeros(R, np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    name = "130 bands, 40 dB"
    freq, mag, phase = (hip._darr(v) for v in CURVES[name])
    assert not nu.update_busy()
    nu.render_eq_async(0, 1, R, *CURVES[name], mode="minimum")
    answers = [L.bfhip_nupc_set_coeff(h, 0, 1),
               L.bfhip_nupc_render_eq_mode_async(h, 0, 1, R, 130, freq, mag, phase, MINIMUM),
               L.bfhip_nupc_render_eq_mode_async(h, 0, 1, R, 130, freq, mag, phase, LINEAR),
               L.bfhip_nupc_render_eq_mode(h, 8, 130, freq, mag, phase, MINIMUM, po),
               L.bfhip_nupc_render_eq_mode(h, 8, 130, freq, mag, phase, LINEAR, po)]
    assert nu.update_busy(), "the rewrite was over before the calls were made: nothing was tested"
    assert answers == [ESTATE] * 5
    assert nu.update_wait() == 0 and nu.update_result() == 0 and not nu.update_busy() and not np.any(out)
    # the set holds the render: a pulse through it, hard switch at frame 0, is the model's taps, and
    # the first block carries most of their energy
    nu.set_crossfade(0)
    nu.set_coeff(0, 1)
    x = np.zeros((nu.L0, 1), np.float32)
    x[0] = 1.0
    y = np.frombuffer(nu.block(x)[1].tobytes(), np.float32)
    assert nu.switch_frame() == 0
    want = _model(R, name)
    assert np.sum(want[:nu.L0] ** 2) >= 0.9 * np.sum(want ** 2)
    assert cases.rel_rms(y, want[:nu.L0]) <= TOL[4]


# ---------------------------------------------------------------- 5: validation

def _convolver_of(hip, twin, reserve_min):
    """the twin's convolver again, not yet run"""
    nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
    nu.set_interleaved(0, FF[4])
    nu.set_interleaved(1, "S24_4LE")
    nu.reserve_update()
    nu.reserve_eq(256)
    if reserve_min:
        nu.reserve_eq_minimum()
    nu.add_filter(0, 0, twin.h[0])
    assert nu.add_coeff(0, twin.h[1]) == 1
    nu.finalize()
    return nu


def _does_what_its_twin_does(nu, twin, curve):
    """after the failed calls: a linear render into the idle set and a switch, the twin's bytes"""
    got = []
    for b in range(SMALL["n_blocks"]):
        if b == SMALL["b_render"]:
            nu.render_eq_async(0, 1, 256, *curve)
            assert nu.update_wait() == 0
        if b == SMALL["b_switch"]:
            nu.set_coeff(0, 1)
        got.append(nu.block(twin.x[b * nu.L0:(b + 1) * nu.L0])[1])
    assert np.array_equal(np.concatenate(got), twin.raw)


def test_argument_and_state_errors_change_nothing(hip):
    L = hip.lib()
    twin = Run(hip, 4, SMALL, "S24_4LE", "eq", mode="linear", curve="knot on a bin")
    nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
    nu.set_interleaved(0, FF[4])
    nu.set_interleaved(1, "S24_4LE")
    h = nu.h
    nu.reserve_update()
    assert L.bfhip_nupc_reserve_eq_minimum(h) == ESTATE                    # before reserve_eq
    assert b"reserve_eq" in L.bfhip_nupc_last_error()
    nu.reserve_eq(256)
    nu.reserve_eq_minimum()
    nu.add_filter(0, 0, twin.h[0])
    assert nu.add_coeff(0, twin.h[1]) == 1
    nu.finalize()
    assert L.bfhip_nupc_reserve_eq_minimum(h) == ESTATE                    # after finalize
    good = CURVES["knot on a bin"]
    before = nu.render_eq(256, *good)
    out = np.zeros(512, np.float32)
    po = out.ctypes.data_as(C.c_void_p)

    def both(taps, curve, mode, filt=0, coeff=1):
        n_bands = len(curve[0])
        f, m, p = (hip._darr(list(v)) for v in curve)
        r = (L.bfhip_nupc_render_eq_mode_async(h, filt, coeff, taps, n_bands, f, m, p, mode),
             L.bfhip_nupc_render_eq_mode(h, taps, n_bands, f, m, p, mode, po))
        assert not nu.update_busy() and not np.any(out)
        return r

    f, m, p = (list(v) for v in good)
    for name, mags in {"zero": [1.0, 0.0, 0.5, 1.5], "negative zero": [1.0, -0.0, 0.5, 1.5], "negative": [1.0, -0.5, 0.5, 1.5],
                       "zero at 0": [0.0, 2.0, 0.5, 1.5], "zero at 0.5": [1.0, 2.0, 0.5, 0.0],
                       "NaN": [1.0, float("nan"), 0.5, 1.5], "Inf": [1.0, float("inf"), 0.5, 1.5]}.items():
        assert both(256, (f, mags, p), MINIMUM) == (EINVAL, EINVAL), name
    fz, mz, pz = (hip._darr(v) for v in (f, [1.0, 0.0, 0.5, 1.5], p))       # linear mode takes a zero knot, as before
    assert L.bfhip_nupc_render_eq_mode(h, 256, 4, fz, mz, pz, LINEAR, po) == 0 and np.any(out)
    out[:] = 0
    for mode in (2, -1, 256):
        assert both(256, good, mode) == (EINVAL, EINVAL), mode
        assert b"mode" in L.bfhip_nupc_last_error()
    for taps in (0, 4, 100, 512):
        assert both(taps, good, MINIMUM) == (EINVAL, EINVAL), taps
    fa, ma, pa = (hip._darr(v) for v in good)
    assert L.bfhip_nupc_render_eq_mode(h, 256, 4, fa, ma, pa, MINIMUM, None) == EINVAL
    assert L.bfhip_nupc_render_eq_mode_async(h, 0, 0, 256, 4, fa, ma, pa, MINIMUM) == ESTATE     # live
    assert not nu.update_busy() and nu.update_result() == 0
    assert np.array_equal(nu.render_eq(256, *good), before)
    _does_what_its_twin_does(nu, twin, good)


def test_minimum_mode_without_its_reservation(hip):
    L = hip.lib()
    twin = Run(hip, 4, SMALL, "S24_4LE", "eq", mode="linear", curve="knot on a bin")
    nu, good = _convolver_of(hip, twin, reserve_min=False), CURVES["knot on a bin"]
    before = nu.render_eq(256, *good)
    f, m, p = (hip._darr(v) for v in good)
    out = np.zeros(256, np.float32)
    assert L.bfhip_nupc_render_eq_mode_async(nu.h, 0, 1, 256, 4, f, m, p, MINIMUM) == ESTATE
    assert b"reserve_eq_minimum" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_render_eq_mode(nu.h, 256, 4, f, m, p, MINIMUM, out.ctypes.data_as(C.c_void_p)) == ESTATE
    assert not nu.update_busy() and not np.any(out)
    assert np.array_equal(nu.render_eq(256, *good), before)
    assert np.array_equal(before, twin.nu.render_eq(256, *good))
    _does_what_its_twin_does(nu, twin, good)
