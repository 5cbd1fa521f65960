"""GPU: equaliser curves rendered ONTO a base impulse response (bfhip_nupc_reserve_eq_base / _set_eq_base /
_render_eq_base_async / _render_eq_base, include/bfhip_nupc.h; brutefir_amd/csrc/eq_apply.h).

What must hold: the synchronous call is the float64 truncated convolution (tests/eq_base_ref.py) of the
base with the taps render_eq returns, at the project's parity bars, float32 1e-5 / float64 1e-12 relative
RMS, for one partial window, R not dividing T, many windows with a partial last one, the LDS limit
R = 8192 and the room-correction length; it is a pure function of its arguments; without set_eq_base
the base is add_filter's taps; a flat curve gives the base back (minimum mode) or the base R/2 frames
later (linear mode); a render into an idle set followed by a switch has the BYTES of
update_coeff_async with the synchronous call's array, and the output after the switch is the float64
model's (tests/nupc_ref.py); the reservation alone, and a render into an idle set before the switch,
change no output byte; every call made while a rewrite is in flight answers BFHIP_ESTATE; and every
argument and state error answers its code and changes nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import eq_base_ref
import eq_minphase_ref
import eq_ref
import nupc_ref

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
DT = {4: np.float32, 8: np.float64}
EINVAL, ESTATE = -1, -5
LINEAR, MINIMUM = 0, 1
MODES = {"linear": LINEAR, "minimum": MINIMUM}
CURVES = {"flat": eq_ref.flat(), "130 bands": eq_ref.random_bands(130, 7), "knot on a bin": eq_ref.knot_on_a_bin(),
          "130 bands, 40 dB": eq_ref.random_bands(130, 3, db=40.0)}
TWO = ("130 bands", "130 bands, 40 dB")
# schedule, T, the largest render length reserved, the lengths rendered.  ([16, 32, 64], [2, 2, 4]), the schedule of
# tests/test_gpu_nupc_eq_minphase.py's SMALL plan, has 352 taps; 448 taps with R = 256 is ([16, 32, 64], [2, 3, 5]):
# both are one partial window of 512
S48 = dict(sched=([8, 16], [2, 2]), T=48, max_taps=32, R=(8, 32))
S352 = dict(sched=([16, 32, 64], [2, 2, 4]), T=352, max_taps=256, R=(256,))
S448 = dict(sched=([16, 32, 64], [2, 3, 5]), T=448, max_taps=256, R=(256,))
S21760 = dict(sched=([64, 256, 1024, 4096], [4, 4, 4, 4]), T=21760, max_taps=16384, R=(8, 64, 2048, 8192))
ROOM = dict(sched=([16384], [64]), T=1048576, max_taps=8192, R=(8192,))
# schedule, blocks run, block the render starts before, block the switch is requested before, render length
SMALL = dict(sched=([16, 32, 64], [2, 2, 4]), n_blocks=60, b_render=3, b_switch=12, R=256)
MID = dict(sched=([32, 128, 512], [4, 4, 4]), n_blocks=130, b_render=3, b_switch=12, R=1024)      # segments 1 and 2 run in the background


def _noise(seed, n, dt):
    return (np.random.default_rng(seed).standard_normal(n) / np.sqrt(n)).astype(dt)


@functools.lru_cache(maxsize=None)
def _model(R, name, mode):
    taps = (eq_minphase_ref if mode == "minimum" else eq_ref).render(R, *CURVES[name])
    taps.setflags(write=False)
    return taps


_renderers = {}


def _renderer(hip, rs, plan_name):
    """one convolver per precision and schedule for the tests that only make synchronous calls on it:
    one filter of T/2 taps with a second set, every reservation"""
    plan = globals()[plan_name]
    if (rs, plan_name) not in _renderers:
        nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, 1, 1)
        assert nu.taps == plan["T"]
        nu.reserve_update()
        nu.reserve_eq(plan["max_taps"])
        nu.reserve_eq_minimum()
        nu.h0 = _noise(1, plan["T"] // 2, DT[rs])
        nu.add_filter(0, 0, nu.h0)
        assert nu.add_coeff(0, _noise(2, 32, DT[rs])) == 1
        nu.reserve_eq_base(0)
        nu.finalize()
        _renderers[(rs, plan_name)] = nu
    return _renderers[(rs, plan_name)]


def _bases(T, R, dt):
    full = _noise(20 + R, T, dt)
    return {"full-length noise": full, "noise with R trailing zeros": np.concatenate([full[:T - R], np.zeros(R, dt)])}


# ---------------------------------------------------------------- 1: the kernel alone

def _kernel_alone(hip, rs, plan_name, R, apply):
    nu = _renderer(hip, rs, plan_name)
    T = nu.taps
    for bname, base in _bases(T, R, DT[rs]).items():
        nu.set_eq_base(0, base)
        for name in TWO:
            for mode in MODES:
                e = nu.render_eq(R, *CURVES[name], mode=mode)
                got = nu.render_eq_base(0, R, *CURVES[name], mode=mode)
                assert got.dtype == DT[rs] and got.shape == (T,)
                want = apply(base.astype(np.float64), e.astype(np.float64), T)
                err = cases.rel_rms(got, want)
                print("rs %d T %d R %d %s, %s, %s: rel rms %.3g (limit %g)" % (rs, T, R, bname, name, mode, err, TOL[rs]))
                assert err <= TOL[rs], (bname, name, mode)
                assert np.array_equal(got, nu.render_eq_base(0, R, *CURVES[name], mode=mode)), (bname, name, mode)   # same arguments, same bytes


@pytest.mark.parametrize("plan_name,R", [(p, R) for p in ("S48", "S352", "S448", "S21760") for R in globals()[p]["R"]])
@pytest.mark.parametrize("rs", [4, 8])
def test_render_onto_a_base_is_the_truncated_convolution(hip, rs, plan_name, R):
    _kernel_alone(hip, rs, plan_name, R, eq_base_ref.apply)


def test_render_onto_a_base_of_the_room_correction_length(hip):
    _kernel_alone(hip, 4, "ROOM", 8192, eq_base_ref.apply_fft)


def test_truncation_is_exercised_by_the_full_length_base():
    """the two bases differ behind T - R, so the full-length one has a tail that the truncation cuts"""
    T, R = 48, 8
    b = _bases(T, R, np.float64)
    e = np.ones(R)
    y = [eq_base_ref.apply(v, e, T) for v in b.values()]
    assert np.array_equal(y[0][:T - R], y[1][:T - R]) and not np.array_equal(y[0][T - R:], y[1][T - R:])
    assert len(np.convolve(b["full-length noise"], e)) > T


# ---------------------------------------------------------------- 2: the default base, a flat curve

@pytest.mark.parametrize("rs", [4, 8])
def test_default_base_is_add_filters_taps(hip, rs):
    nu = hip.Nupc(*S448["sched"], rs, 1, 1)
    nu.reserve_update()
    nu.reserve_eq(256)
    nu.reserve_eq_minimum()
    h0 = _noise(1, 200, DT[rs])                                # shorter than T: zero-padded
    nu.add_filter(0, 0, h0, 0.5, 3.0)                          # the scales are not part of the base
    assert nu.add_coeff(0, _noise(2, 64, DT[rs])) == 1
    nu.reserve_eq_base(0)
    nu.finalize()
    first = {m: nu.render_eq_base(0, 256, *CURVES["130 bands"], mode=m) for m in MODES}
    nu.set_eq_base(0, h0)
    for m in MODES:
        assert np.any(first[m]) and np.array_equal(first[m], nu.render_eq_base(0, 256, *CURVES["130 bands"], mode=m)), m
        want = eq_base_ref.apply(h0.astype(np.float64), nu.render_eq(256, *CURVES["130 bands"], mode=m).astype(np.float64), nu.taps)
        assert cases.rel_rms(first[m], want) <= TOL[rs], m


@pytest.mark.parametrize("plan_name,R", [("S48", 32), ("S21760", 64), ("S21760", 8192)])
@pytest.mark.parametrize("rs", [4, 8])
def test_flat_curve_gives_the_base_back_or_delays_it_by_half_its_length(hip, rs, plan_name, R):
    nu = _renderer(hip, rs, plan_name)
    T = nu.taps
    base = _noise(30, T, DT[rs])
    nu.set_eq_base(0, base)
    b = base.astype(np.float64)
    for mode, shift in (("minimum", 0), ("linear", R // 2)):
        got = nu.render_eq_base(0, R, *CURVES["flat"], mode=mode)
        want = np.concatenate([np.zeros(shift), b[:T - shift]])
        err = cases.rel_rms(got, want)
        print("rs %d T %d R %d %s: rel rms against the base %d frames later %.3g (limit %g)" % (rs, T, R, mode, shift, err, TOL[rs]))
        assert err <= TOL[rs], mode


# ---------------------------------------------------------------- runs with a switch onto a rendered set

class Run:
    """one filter with two sets of flat noise and a base of its own; `how` rewrites set 1 before block
    b_render: "base" render_eq_base_async in `mode`, "upload" update_coeff_async with the array
    render_eq_base returns in `mode`, None not at all; the switch 0 -> 1 is requested before block b_switch"""

    def __init__(self, hip, rs, plan, out_fmt, how, mode="minimum", reserve_base=True, wait_at_switch=False,
                 curve="130 bands", switch=True, set_base=True):
        dt = DT[rs]
        self.nu = nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, 1, 1)
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, out_fmt)
        nu.reserve_update()
        nu.reserve_eq(plan["R"])
        nu.reserve_eq_minimum()
        self.h = [_noise(11, nu.taps, dt), _noise(12, nu.taps, dt)]
        self.base = _noise(13, nu.taps - plan["R"], dt)          # R trailing zeros: nothing is truncated
        nu.add_filter(0, 0, self.h[0])
        assert nu.add_coeff(0, self.h[1]) == 1
        if reserve_base:
            nu.reserve_eq_base(0)
        nu.finalize()
        if reserve_base and set_base:
            nu.set_eq_base(0, self.base)
        self.L0, R = nu.L0, plan["R"]
        self.x = (np.random.default_rng(5).standard_normal((plan["n_blocks"] * nu.L0, 1)) * 0.02).astype(dt)
        got = []
        for b in range(plan["n_blocks"]):
            if b == plan["b_render"] and how == "base":
                nu.render_eq_base_async(0, 1, R, *CURVES[curve], mode=mode)
                if not wait_at_switch:
                    assert nu.update_wait() == 0
            if b == plan["b_render"] and how == "upload":
                nu.update_coeff_async(0, 1, nu.render_eq_base(0, R, *CURVES[curve], mode=mode))
                assert nu.update_wait() == 0
            if b == plan["b_switch"] and switch:
                if how == "base" and wait_at_switch:
                    assert nu.update_wait() == 0
                nu.set_coeff(0, 1)
            got.append(nu.block(self.x[b * nu.L0:(b + 1) * nu.L0]))
        self.status = [s for s, _ in got]
        self.raw = np.concatenate([r for _, r in got])
        self.t_sw = nu.switch_frame()


# ---------------------------------------------------------------- 3: same bits as the upload path

@pytest.mark.parametrize("rs,plan,out_fmt,mode", [(4, SMALL, "S24_4LE", "minimum"), (4, SMALL, "S24_4LE", "linear"),
                                                  (8, MID, "FLOAT64_LE", "minimum")], ids=["f32 small min", "f32 small lin", "f64 background"])
def test_render_onto_a_base_into_a_set_has_the_bits_of_the_upload(hip, rs, plan, out_fmt, mode):
    a = Run(hip, rs, plan, out_fmt, "base", mode=mode)
    b = Run(hip, rs, plan, out_fmt, "upload", mode=mode)
    assert a.t_sw == b.t_sw and a.t_sw > 0
    assert (a.t_sw + a.L0 + a.nu.taps) < len(a.x), "the run must go on beyond the switch window"
    assert a.status == b.status
    assert np.array_equal(a.raw, b.raw)
    assert np.any(a.raw[(a.t_sw + a.L0) * a.nu.out_bytes // a.L0:])


# ---------------------------------------------------------------- 4: against the float64 model end to end

@pytest.mark.parametrize("mode", ["minimum", "linear"])
@pytest.mark.parametrize("rs", [4, 8])
def test_output_after_the_switch_is_the_models(hip, rs, mode):
    r = Run(hip, rs, SMALL, FF[rs], "base", mode=mode)
    L0, n, T = r.L0, len(r.x), r.nu.taps
    new = eq_base_ref.apply(r.base.astype(np.float64), _model(SMALL["R"], "130 bands", mode), T)
    x = r.x.astype(np.float64)
    ys = [nupc_ref.convolve(x, [(0, 0, h, 1.0, 1.0)], 1) for h in (r.h[0], new)]
    want = nupc_ref.switched(ys, [(r.t_sw, L0, 1)])
    fmts = [nupc_ref.fmt(FF[rs])]
    want = nupc_ref.decode(nupc_ref.encode(want, fmts, L0)[0], fmts, n)
    got = nupc_ref.decode(r.raw, fmts, n)
    err = cases.rel_rms(got, want)
    print("rs %d %s: rel rms whole run %.3g (limit %g)" % (rs, mode, err, TOL[rs]))
    assert err <= TOL[rs]
    assert r.t_sw > 0 and cases.rel_rms(got[:r.t_sw], ys[0][:r.t_sw]) <= TOL[rs]       # before t_sw: the old set's
    t = r.t_sw + L0                                                                  # behind the fade: the new set alone
    err = cases.rel_rms(got[t:], ys[1][t:])
    print("rs %d %s: rel rms behind the fade %.3g (limit %g)" % (rs, mode, err, TOL[rs]))
    assert t < n - L0 and err <= TOL[rs]
    assert cases.rel_rms(got[t:], ys[0][t:]) > 0.5                                   # and not the old one


# ---------------------------------------------------------------- 5: no side effects

def test_the_reservation_alone_changes_no_byte(hip):
    a = Run(hip, 4, SMALL, "S24_4LE", None, reserve_base=True)
    b = Run(hip, 4, SMALL, "S24_4LE", None, reserve_base=False)
    assert a.t_sw == b.t_sw and a.status == b.status and np.array_equal(a.raw, b.raw)


@pytest.mark.parametrize("rs,plan", [(4, SMALL), (8, MID)], ids=["f32 small", "f64 background"])
def test_render_into_an_idle_set_changes_no_byte_before_the_switch(hip, rs, plan):
    plan = dict(plan, n_blocks=plan["b_switch"] + 30)
    a = Run(hip, rs, plan, FF[rs], "base", wait_at_switch=True, switch=False)      # rendered, never switched to
    b = Run(hip, rs, plan, FF[rs], None, switch=False)
    assert a.nu.update_wait() == 0
    assert np.array_equal(a.raw, b.raw)
    a = Run(hip, rs, plan, FF[rs], "base", wait_at_switch=True)                    # the render beside the periods
    b = Run(hip, rs, plan, FF[rs], None)
    cut = a.t_sw // a.L0 * a.nu.out_bytes
    assert a.t_sw == b.t_sw and cut > 0 and np.array_equal(a.raw[:cut], b.raw[:cut])


def test_calls_while_a_render_onto_a_base_is_in_flight(hip):
    """1 048 576 taps into 64 partitions of 16384.  Each call is made directly behind an asynchronous
    render's return, and busy is looked at behind the call: still 1 means that the call was made while
    the rewrite was in flight, and only such a call's answer counts.  The device needs some 80 us behind
    the return and a call a few, so the first attempt counts as a rule; that every call was seen in
    flight within a few attempts is asserted."""
    L = hip.lib()
    nu = _renderer(hip, 4, "ROOM")
    h, T, R = nu.h, nu.taps, 8192
    name = "130 bands, 40 dB"
    base = _noise(40, T, np.float32)
    nu.set_eq_base(0, base)
    want = nu.render_eq_base(0, R, *CURVES[name], mode="minimum")
    out = np.zeros(T, np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    other = _noise(41, T, np.float32)
    pt = other.ctypes.data_as(C.c_void_p)
    freq, mag, phase = (hip._darr(v) for v in CURVES[name])
    calls = {"set_eq_base": lambda: L.bfhip_nupc_set_eq_base(h, 0, pt, T),
             "render_eq_base": lambda: L.bfhip_nupc_render_eq_base(h, 0, R, 130, freq, mag, phase, MINIMUM, po),
             "render_eq_base_async": lambda: L.bfhip_nupc_render_eq_base_async(h, 0, 1, R, 130, freq, mag, phase, MINIMUM),
             "update_coeff_async": lambda: L.bfhip_nupc_update_coeff_async(h, 0, 1, pt, T),
             "set_coeff": lambda: L.bfhip_nupc_set_coeff(h, 0, 1)}
    for what, call in calls.items():
        for attempt in range(10):
            assert not nu.update_busy()
            nu.render_eq_base_async(0, 1, R, *CURVES[name], mode="minimum")
            answer = call()
            seen_in_flight = nu.update_busy()
            assert nu.update_wait() == 0
            if seen_in_flight:
                break
            # the rewrite was over before the call: the call was entitled to succeed; put back what it changed
            out[:] = 0
            nu.set_eq_base(0, base)
            nu.set_coeff(0, 0)                                  # a group that changes no set commits no switch
        print("%s: answer %d on attempt %d" % (what, answer, attempt + 1))
        assert seen_in_flight, "the rewrite was never in flight behind %s: nothing was tested" % what
        assert answer == ESTATE, what
        assert nu.update_result() == 0 and not nu.update_busy() and not np.any(out)
    assert np.array_equal(nu.render_eq_base(0, R, *CURVES[name], mode="minimum"), want)       # the base is as it was
    # the set holds the render: a pulse through it, hard switch at frame 0, is the first block of the array
    nu.set_crossfade(0)
    nu.set_coeff(0, 1)
    x = np.zeros((nu.L0, 1), np.float32)
    x[0] = 1.0
    y = np.frombuffer(nu.block(x)[1].tobytes(), np.float32)
    assert nu.switch_frame() == 0
    assert np.any(want[:nu.L0]) and cases.rel_rms(y, want[:nu.L0]) <= TOL[4]


# ---------------------------------------------------------------- 6: validation

def _convolver(hip, twin, reserve_min=True, reserve_base=True, before_finalize=None):
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
    if reserve_base:
        nu.reserve_eq_base(0)
    if before_finalize:
        before_finalize(nu)
    nu.finalize()
    if reserve_base:
        nu.set_eq_base(0, twin.base)
    return nu


def _does_what_its_twin_does(nu, twin, curve, how="base"):
    """after the failed calls: the twin's render into the idle set and its switch, the twin's bytes"""
    got = []
    for b in range(SMALL["n_blocks"]):
        if b == SMALL["b_render"]:
            if how == "base":
                nu.render_eq_base_async(0, 1, 256, *curve)
            else:
                nu.render_eq_async(0, 1, 256, *curve)
            assert nu.update_wait() == 0
        if b == SMALL["b_switch"]:
            nu.set_coeff(0, 1)
        got.append(nu.block(twin.x[b * nu.L0:(b + 1) * nu.L0])[1])
    assert np.array_equal(np.concatenate(got), twin.raw)


def _both(hip, nu, out, taps, curve, mode, filt=0, coeff=1):
    L, n_bands = hip.lib(), len(curve[0])
    f, m, p = (hip._darr(list(v)) for v in curve)
    r = (L.bfhip_nupc_render_eq_base_async(nu.h, filt, coeff, taps, n_bands, f, m, p, mode),
         L.bfhip_nupc_render_eq_base(nu.h, filt, taps, n_bands, f, m, p, mode, out.ctypes.data_as(C.c_void_p)))
    assert not nu.update_busy() and not np.any(out)
    return r


def test_argument_and_state_errors_change_nothing(hip):
    L = hip.lib()
    good = CURVES["knot on a bin"]
    twin = Run(hip, 4, SMALL, "S24_4LE", "base", mode="linear", curve="knot on a bin")
    nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
    nu.set_interleaved(0, FF[4])
    nu.set_interleaved(1, "S24_4LE")
    h = nu.h
    out = np.zeros(nu.taps, np.float32)
    nu.reserve_update()
    nu.add_filter(0, 0, twin.h[0])
    assert nu.add_coeff(0, twin.h[1]) == 1
    assert L.bfhip_nupc_reserve_eq_base(h, 0) == ESTATE                     # before reserve_eq
    assert b"reserve_eq" in L.bfhip_nupc_last_error()
    nu.reserve_eq(256)
    nu.reserve_eq_minimum()
    for filt in (-1, 1, 7):
        assert L.bfhip_nupc_reserve_eq_base(h, filt) == EINVAL, filt        # no such filter
    nu.reserve_eq_base(0)
    pb = twin.base.ctypes.data_as(C.c_void_p)
    assert L.bfhip_nupc_set_eq_base(h, 0, pb, len(twin.base)) == ESTATE     # before finalize
    assert _both(hip, nu, out, 256, good, LINEAR) == (ESTATE, ESTATE)
    nu.finalize()
    assert L.bfhip_nupc_reserve_eq_base(h, 0) == ESTATE                     # after finalize
    nu.set_eq_base(0, twin.base)
    before = nu.render_eq_base(0, 256, *good)

    for taps in (0, 4, 12, 100, 512, 16384):                               # not a power of two >= 8, above max_taps
        for mode in (LINEAR, MINIMUM):
            assert _both(hip, nu, out, taps, good, mode) == (EINVAL, EINVAL), taps
    for mode in (2, -1):
        assert _both(hip, nu, out, 256, good, mode) == (EINVAL, EINVAL), mode
    f, m, p = (list(v) for v in good)
    assert _both(hip, nu, out, 256, (f, [1.0, 0.0, 0.5, 1.5], p), MINIMUM) == (EINVAL, EINVAL)     # a zero magnitude
    assert _both(hip, nu, out, 256, (f, [1.0, float("nan"), 0.5, 1.5], p), LINEAR) == (EINVAL, EINVAL)
    assert _both(hip, nu, out, 256, (f[:1], m[:1], p[:1]), LINEAR) == (EINVAL, EINVAL)
    for filt in (-1, 1):
        assert _both(hip, nu, out, 256, good, LINEAR, filt=filt) == (EINVAL, EINVAL), filt
    fa, ma, pa = (hip._darr(v) for v in good)
    assert L.bfhip_nupc_render_eq_base(h, 0, 256, 4, fa, ma, pa, LINEAR, None) == EINVAL
    assert L.bfhip_nupc_render_eq_base_async(h, 0, 2, 256, 4, fa, ma, pa, LINEAR) == EINVAL         # no such set
    assert L.bfhip_nupc_render_eq_base_async(h, 0, 0, 256, 4, fa, ma, pa, LINEAR) == ESTATE         # live
    # set_eq_base: lengths, a NaN, an Inf
    bad = twin.base.copy()
    for n_taps in (0, -1, nu.taps + 1):
        assert L.bfhip_nupc_set_eq_base(h, 0, pb, n_taps) == EINVAL, n_taps
    assert L.bfhip_nupc_set_eq_base(h, 0, None, 8) == EINVAL and L.bfhip_nupc_set_eq_base(h, 1, pb, 8) == EINVAL
    for v in (np.nan, np.inf, -np.inf):
        bad[17] = v
        assert L.bfhip_nupc_set_eq_base(h, 0, bad.ctypes.data_as(C.c_void_p), len(bad)) == EINVAL
        assert L.bfhip_nupc_last_error() == b"NaN or Inf value among coefficients."
    assert not nu.update_busy() and nu.update_result() == 0
    assert np.array_equal(nu.render_eq_base(0, 256, *good), before)
    _does_what_its_twin_does(nu, twin, good)
    # set 1 is live now, and set 0 (idle, full length) is queued once the switch back has been asked for
    assert L.bfhip_nupc_render_eq_base_async(h, 0, 1, 256, 4, fa, ma, pa, LINEAR) == ESTATE
    assert not nu.switch_busy()
    nu.set_coeff(0, 0)
    assert L.bfhip_nupc_render_eq_base_async(h, 0, 0, 256, 4, fa, ma, pa, LINEAR) == ESTATE
    assert b"queued" in L.bfhip_nupc_last_error() and not nu.update_busy()


def test_eq_taps_above_what_one_workgroup_transforms(hip):
    """max_taps is 16384 here: the plain render takes 16384 taps, the render onto a base stops at 8192"""
    nu = _renderer(hip, 4, "S21760")
    out = np.zeros(nu.taps, np.float32)
    before = nu.render_eq_base(0, 8192, *CURVES["knot on a bin"])
    assert _both(hip, nu, out, 16384, CURVES["knot on a bin"], LINEAR) == (EINVAL, EINVAL)
    assert b"8192" in hip.lib().bfhip_nupc_last_error()
    assert np.any(nu.render_eq(16384, *CURVES["knot on a bin"]))
    assert np.array_equal(nu.render_eq_base(0, 8192, *CURVES["knot on a bin"]), before)


def test_without_the_reservations(hip):
    L = hip.lib()
    good = CURVES["knot on a bin"]
    fa, ma, pa = (hip._darr(v) for v in good)
    # no reserve_eq_base at all: the plain render's twin
    twin = Run(hip, 4, SMALL, "S24_4LE", None, reserve_base=False, switch=False)
    nu = _convolver(hip, twin, reserve_base=False)
    out = np.zeros(nu.taps, np.float32)
    assert L.bfhip_nupc_set_eq_base(nu.h, 0, twin.base.ctypes.data_as(C.c_void_p), len(twin.base)) == ESTATE
    assert b"reserve_eq_base" in L.bfhip_nupc_last_error()
    assert _both(hip, nu, out, 256, good, LINEAR) == (ESTATE, ESTATE)
    assert b"reserve_eq_base" in L.bfhip_nupc_last_error()
    got = [nu.block(twin.x[b * nu.L0:(b + 1) * nu.L0])[1] for b in range(SMALL["n_blocks"])]
    assert np.array_equal(np.concatenate(got), twin.raw)
    # minimum mode without reserve_eq_minimum
    twin = Run(hip, 4, SMALL, "S24_4LE", "base", mode="linear", curve="knot on a bin")
    nu = _convolver(hip, twin, reserve_min=False)
    before = nu.render_eq_base(0, 256, *good)
    assert _both(hip, nu, out, 256, good, MINIMUM) == (ESTATE, ESTATE)
    assert b"reserve_eq_minimum" in L.bfhip_nupc_last_error()
    assert np.array_equal(nu.render_eq_base(0, 256, *good), before)
    _does_what_its_twin_does(nu, twin, good)


def test_set_0_must_cover_every_partition(hip):
    """y spans the whole schedule: set 0 of a filter added with fewer taps cannot take it, however idle"""
    L = hip.lib()
    good = CURVES["knot on a bin"]
    fa, ma, pa = (hip._darr(v) for v in good)
    x = (np.random.default_rng(5).standard_normal((SMALL["n_blocks"] * 16, 1)) * 0.02).astype(np.float32)
    raws = {}
    for n0, answer in ((100, EINVAL), (352, 0)):
        for touch in (False, True):
            nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
            nu.reserve_update()
            nu.reserve_eq(256)
            assert n0 <= nu.taps == 352
            nu.add_filter(0, 0, _noise(11, n0, np.float32))
            assert nu.add_coeff(0, _noise(12, nu.taps, np.float32)) == 1
            nu.reserve_eq_base(0)
            nu.finalize()
            nu.set_coeff(0, 1)
            got = []
            for b in range(SMALL["n_blocks"]):
                if b == 40 and touch:                          # the switch is over: set 0 is idle
                    assert not nu.switch_busy()
                    assert L.bfhip_nupc_render_eq_base_async(nu.h, 0, 0, 256, 4, fa, ma, pa, LINEAR) == answer
                    if answer == EINVAL:
                        assert b"set 0" in L.bfhip_nupc_last_error() and not nu.update_busy()
                    else:
                        assert nu.update_wait() == 0
                got.append(nu.block(x[b * 16:(b + 1) * 16])[1])
            raws[(n0, touch)] = np.concatenate(got)
        assert np.array_equal(raws[(n0, True)], raws[(n0, False)]), n0      # nothing changed; an idle set's rewrite is not heard
