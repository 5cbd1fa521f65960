"""GPU: equaliser curves rendered on the device (bfhip_nupc_reserve_eq / _render_eq_async /
_render_eq, include/bfhip_nupc.h).

What must hold: the render alone is the float64 model's (tests/eq_ref.py) at the project's parity
bars, float32 1e-5 / float64 1e-12 relative RMS, on the one-workgroup path (R <= 16384) and on the
big-FFT sequence with one combine pass of radix 2, 4, 8 and with two passes; a render is a pure
function of its arguments; render_eq_async into an idle set followed by a switch has the BYTES of
update_coeff_async with the array render_eq returned; the output after the switch is the float64
model's (tests/nupc_ref.py, the bars of tests/test_gpu_nupc_rewrite.py); a reservation alone, and a
render into an idle set before the switch, change no output byte; and every argument and state
error of the header answers its code and changes nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import eq_ref
import nupc_ref

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
DT = {4: np.float32, 8: np.float64}
EINVAL, ESTATE = -1, -5
CURVES = {"flat": eq_ref.flat(), "130 bands": eq_ref.random_bands(130, 7), "knot on a bin": eq_ref.knot_on_a_bin(),
          "skipped band": eq_ref.skipped_band()}
LENGTHS = [8, 64, 4096, 16384, 32768, 65536, 131072, 262144]
# schedule, blocks run, block the render starts before, block the switch is requested before, render length
SMALL = dict(sched=([16, 32, 64], [2, 2, 4]), n_blocks=60, b_render=3, b_switch=12, R=256)
BIG = dict(sched=([64, 256, 1024, 4096, 16384], [4, 4, 4, 4, 1]), n_blocks=1300, b_render=3, b_switch=40, R=32768)


def _noise(seed, n, dt):
    return (np.random.default_rng(seed).standard_normal(n) / np.sqrt(n)).astype(dt)


@functools.lru_cache(maxsize=None)
def _model(R, name):
    taps = eq_ref.render(R, *CURVES[name])
    taps.setflags(write=False)
    return taps


_renderers = {}


def _make_renderer(hip, rs):
    """a single 16384-frame segment, 1 048 576 taps in float32 and 262 144 in float64, one filter with
    a second set to render into"""
    nu = hip.Nupc([16384], [64 if rs == 4 else 16], rs, 1, 1)
    nu.reserve_update()
    nu.reserve_eq(nu.taps)
    nu.add_filter(0, 0, _noise(1, 64, DT[rs]))
    assert nu.add_coeff(0, _noise(2, 64, DT[rs])) == 1
    nu.finalize()
    return nu


def _renderer(hip, rs):
    """one convolver per precision, shared by the tests that only call render_eq on it"""
    if rs not in _renderers:
        _renderers[rs] = _make_renderer(hip, rs)
    return _renderers[rs]


# ---------------------------------------------------------------- 1: the render alone

@pytest.mark.parametrize("R", LENGTHS)
@pytest.mark.parametrize("rs", [4, 8])
def test_render_is_the_float64_model(hip, rs, R):
    nu = _renderer(hip, rs)
    for name, curve in CURVES.items():
        got = nu.render_eq(R, *curve)
        assert got.dtype == DT[rs] and got.shape == (R,)
        err = cases.rel_rms(got, _model(R, name))
        print("rs %d R %d %s: rel rms %.3g (limit %g)" % (rs, R, name, err, TOL[rs]))
        assert err <= TOL[rs], name
        assert np.array_equal(got, nu.render_eq(R, *curve)), name       # a pure function of its arguments


def test_render_of_the_full_room_correction_length(hip):
    nu, R = _renderer(hip, 4), 1048576
    got = nu.render_eq(R, *CURVES["130 bands"])
    err = cases.rel_rms(got, _model(R, "130 bands"))
    print("rs 4 R %d: rel rms %.3g (limit %g)" % (R, err, TOL[4]))
    assert err <= TOL[4]
    assert np.array_equal(got, nu.render_eq(R, *CURVES["130 bands"]))


# ---------------------------------------------------------------- runs with a switch onto a rendered set

class Run:
    """one filter with two sets of flat noise; `how` rewrites set 1 before block b_render:
    "eq" render_eq_async, "upload" update_coeff_async with the array render_eq returns, None not at
    all; the switch 0 -> 1 is requested before block b_switch"""

    def __init__(self, hip, rs, plan, out_fmt, how, reserve_eq=True, wait_at_switch=False, curve="130 bands", switch=True):
        dt = DT[rs]
        self.nu = nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, 1, 1)
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, out_fmt)
        nu.reserve_update()
        if reserve_eq:
            nu.reserve_eq(plan["R"])
        self.h = [_noise(11, nu.taps, dt), _noise(12, nu.taps, dt)]
        nu.add_filter(0, 0, self.h[0])
        assert nu.add_coeff(0, self.h[1]) == 1
        nu.finalize()
        self.L0, R = nu.L0, plan["R"]
        self.x = (np.random.default_rng(5).standard_normal((plan["n_blocks"] * nu.L0, 1)) * 0.02).astype(dt)
        got = []
        for b in range(plan["n_blocks"]):
            if b == plan["b_render"] and how == "eq":
                nu.render_eq_async(0, 1, R, *CURVES[curve])
                if not wait_at_switch:
                    assert nu.update_wait() == 0
            if b == plan["b_render"] and how == "upload":
                nu.update_coeff_async(0, 1, nu.render_eq(R, *CURVES[curve]))
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
def test_render_into_a_set_has_the_bits_of_the_upload(hip, rs, plan, out_fmt):
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


# ---------------------------------------------------------------- 4: no side effects

def test_a_reservation_alone_changes_no_byte(hip):
    a = Run(hip, 4, SMALL, "S24_4LE", None, reserve_eq=True)
    b = Run(hip, 4, SMALL, "S24_4LE", None, reserve_eq=False)
    assert a.t_sw == b.t_sw and np.array_equal(a.raw, b.raw)


@pytest.mark.parametrize("rs,plan", [(4, SMALL), (8, BIG)], ids=["f32 lds", "f64 big"])
def test_render_into_an_idle_set_changes_no_byte_before_the_switch(hip, rs, plan):
    plan = dict(plan, n_blocks=plan["b_switch"] + 20)
    a = Run(hip, rs, plan, FF[rs], "eq", wait_at_switch=True, switch=False)     # rendered, never switched to
    b = Run(hip, rs, plan, FF[rs], None, switch=False)
    assert a.nu.update_wait() == 0
    assert np.array_equal(a.raw, b.raw)
    a = Run(hip, rs, plan, FF[rs], "eq", wait_at_switch=True)                   # the render beside the periods
    b = Run(hip, rs, plan, FF[rs], None)
    cut = a.t_sw // a.L0 * a.nu.out_bytes
    assert a.t_sw == b.t_sw and cut > 0 and np.array_equal(a.raw[:cut], b.raw[:cut])


def test_calls_while_a_render_is_in_flight(hip):
    """1 048 576 taps into 64 partitions of 16384: the host calls below take microseconds, the device
    work does not; that the rewrite was still in flight behind the last of them is asserted"""
    L = hip.lib()
    nu = _make_renderer(hip, 4)
    h, R = nu.h, nu.taps
    taps = _noise(3, 64, np.float32)
    p = taps.ctypes.data_as(C.c_void_p)
    out = np.zeros(R, np.float32)
    freq, mag, phase = (hip._darr(v) for v in CURVES["130 bands"])
    assert not nu.update_busy()
    nu.render_eq_async(0, 1, R, *CURVES["130 bands"])
    answers = [L.bfhip_nupc_set_coeff(h, 0, 1),
               L.bfhip_nupc_render_eq_async(h, 0, 1, R, 130, freq, mag, phase),
               L.bfhip_nupc_update_coeff_async(h, 0, 1, p, 64),
               L.bfhip_nupc_render_eq(h, 8, 130, freq, mag, phase, out.ctypes.data_as(C.c_void_p))]
    assert nu.update_busy(), "the rewrite was over before the calls were made: nothing was tested"
    assert answers == [ESTATE] * 4
    assert nu.update_wait() == 0 and nu.update_result() == 0 and not nu.update_busy() and not np.any(out)
    # the set holds the render: a pulse through it, hard switch at frame 0, is the model's taps; the
    # block around tap R/2 carries their energy
    nu.set_crossfade(0)
    nu.set_coeff(0, 1)
    x = np.zeros((nu.L0, 1), np.float32)
    x[0] = 1.0
    mid = R // 2 // nu.L0
    y = [np.frombuffer(nu.block(x if b == 0 else x * 0)[1].tobytes(), np.float32) for b in range(mid + 1)]
    assert nu.switch_frame() == 0
    want = _model(R, "130 bands")
    assert cases.rel_rms(y[mid], want[mid * nu.L0:(mid + 1) * nu.L0]) <= TOL[4]


# ---------------------------------------------------------------- 5: validation

def _bad_curves():
    f, m, p = (list(v) for v in eq_ref.knot_on_a_bin())
    nan, inf = float("nan"), float("inf")
    many = eq_ref.random_bands(130, 9)
    return {"freq[0] != 0": ([0.01] + f[1:], m, p), "freq[last] != 0.5": (f[:-1] + [0.49], m, p),
            "not ascending": ([0.0, 0.25, 0.25, 0.5], m, p), "descending": ([0.0, 0.3, 0.2, 0.5], m, p),
            "NaN freq": ([0.0, nan, 0.25, 0.5], m, p), "NaN mag": (f, [1.0, nan, 1.0, 1.0], p),
            "negative mag": (f, [1.0, -0.5, 1.0, 1.0], p), "Inf mag": (f, [1.0, inf, 1.0, 1.0], p),
            "NaN phase": (f, m, [0.0, nan, 0.0, 0.0]), "Inf phase": (f, m, [0.0, 0.0, inf, 0.0]),
            "1 band": ([0.0], [1.0], [0.0]),
            "131 bands": tuple(list(v) + [x] for v, x in zip(many, (0.6, 1.0, 0.0)))}


def test_argument_and_state_errors_change_nothing(hip):
    L = hip.lib()
    twin = Run(hip, 4, SMALL, "S24_4LE", "eq", curve="knot on a bin")
    dt = np.float32
    nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
    nu.set_interleaved(0, FF[4])
    nu.set_interleaved(1, "S24_4LE")
    h = nu.h
    assert L.bfhip_nupc_reserve_eq(h, 256) == ESTATE                       # before reserve_update
    nu.reserve_update()
    for bad in (0, 4, 100, 512, -8):                                       # taps() is 352
        assert L.bfhip_nupc_reserve_eq(h, bad) == EINVAL, bad
    nu.reserve_eq(256)
    nu.add_filter(0, 0, twin.h[0])
    assert nu.add_coeff(0, twin.h[1]) == 1
    nu.finalize()
    assert L.bfhip_nupc_reserve_eq(h, 256) == ESTATE                       # after finalize
    out = np.zeros(512, dt)
    po = out.ctypes.data_as(C.c_void_p)

    def both(taps, curve, filt=0, coeff=1):
        n_bands = len(curve[0])
        f, m, p = (hip._darr(list(v)) for v in curve)
        r = (L.bfhip_nupc_render_eq_async(h, filt, coeff, taps, n_bands, f, m, p),
             L.bfhip_nupc_render_eq(h, taps, n_bands, f, m, p, po))
        assert not nu.update_busy() and not np.any(out)
        return r

    good = CURVES["knot on a bin"]
    for taps in (0, 4, 100, 255, 512, -256):
        assert both(taps, good) == (EINVAL, EINVAL), taps
    for name, curve in _bad_curves().items():
        assert both(256, curve) == (EINVAL, EINVAL), name
    f, m, p = (hip._darr(list(v)) for v in good)
    assert L.bfhip_nupc_render_eq_async(h, 0, 1, 256, 4, None, m, p) == EINVAL
    assert L.bfhip_nupc_render_eq(h, 256, 4, f, m, p, None) == EINVAL
    assert L.bfhip_nupc_render_eq_async(h, 1, 1, 256, 4, f, m, p) == EINVAL      # no such filter
    assert L.bfhip_nupc_render_eq_async(h, 0, 2, 256, 4, f, m, p) == EINVAL      # no such set
    assert L.bfhip_nupc_render_eq_async(h, 0, 0, 256, 4, f, m, p) == ESTATE      # live
    assert not nu.update_busy() and nu.update_result() == 0
    # after all of them the convolver does what its twin does, which made none of these calls
    got = []
    for b in range(SMALL["n_blocks"]):
        if b == SMALL["b_render"]:
            nu.render_eq_async(0, 1, 256, *good)
            assert nu.update_wait() == 0
        if b == SMALL["b_switch"]:
            nu.set_coeff(0, 1)
        got.append(nu.block(twin.x[b * nu.L0:(b + 1) * nu.L0])[1])
    assert np.array_equal(np.concatenate(got), twin.raw)


def test_set_0_keeps_add_filter_length(hip):
    L = hip.lib()
    nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
    nu.reserve_update()
    nu.reserve_eq(256)
    nu.add_filter(0, 0, _noise(1, 40, np.float32))            # segment 0 and one 32-partition of segment 1: taps [0, 64)
    assert nu.add_coeff(0, _noise(2, nu.taps, np.float32)) == 1
    nu.finalize()
    nu.set_coeff(0, 1)
    x = np.zeros((nu.L0, 1), np.float32)
    for _ in range(40):
        nu.block(x)
    assert not nu.switch_busy()
    f, m, p = (hip._darr(list(v)) for v in CURVES["flat"])
    assert L.bfhip_nupc_render_eq_async(nu.h, 0, 0, 128, 2, f, m, p) == EINVAL
    assert not nu.update_busy()
    nu.render_eq_async(0, 0, 64, *CURVES["flat"])
    assert nu.update_wait() == 0


def test_without_a_reservation(hip):
    L = hip.lib()
    nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
    nu.reserve_update()
    nu.add_filter(0, 0, _noise(1, nu.taps, np.float32))
    assert nu.add_coeff(0, _noise(2, nu.taps, np.float32)) == 1
    nu.finalize()
    f, m, p = (hip._darr(list(v)) for v in CURVES["flat"])
    out = np.zeros(64, np.float32)
    assert L.bfhip_nupc_render_eq_async(nu.h, 0, 1, 64, 2, f, m, p) == ESTATE
    assert b"reserve_eq" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_render_eq(nu.h, 64, 2, f, m, p, out.ctypes.data_as(C.c_void_p)) == ESTATE
    assert not nu.update_busy() and not np.any(out)
    nu.update_coeff_async(0, 1, _noise(3, nu.taps, np.float32))            # the rewrite itself is as before
    assert nu.update_wait() == 0
