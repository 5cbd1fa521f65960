"""GPU: equaliser curves of more than 8192 taps rendered onto a base impulse response
(bfhip_nupc_reserve_eq_base_long, include/bfhip_nupc.h; the second half of brutefir_amd/csrc/eq_apply.h).
Every convolver here makes the new reservation.

What must hold: the synchronous call is the float64 truncated convolution (tests/eq_base_ref.apply_fft: one
FFT of the whole length, the direct sum takes minutes here) of the base with the taps render_eq returns, at
the project's parity bars, float32 1e-5 / float64 1e-12 relative RMS, for two windows with a partial second
one (the big FFT splits the transform in two), for one whole window, for four windows, for the first length
that needs more than one combine pass, and at the room-correction length; it is a pure function of its
arguments; a flat curve gives the base back (minimum mode) or the base R/2 frames later (linear mode); for
eq_taps <= 8192 the reservation changes no byte, and a convolver without it still stops at 8192; a render
into an idle set followed by a hard switch has the BYTES of update_coeff_async with the synchronous call's
array, and the output from the switch on is the float64 model's (tests/nupc_ref.py); and every argument and
state error answers its code and changes nothing."""
import ctypes as C

import numpy as np
import pytest

import cases
import eq_base_ref
import eq_ref
import nupc_ref

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
DT = {4: np.float32, 8: np.float64}
EINVAL, ESTATE = -1, -5
LINEAR, MINIMUM = 0, 1
MODES = ("linear", "minimum")
CURVES = {"flat": eq_ref.flat(), "130 bands": eq_ref.random_bands(130, 7), "130 bands, 40 dB": eq_ref.random_bands(130, 3, db=40.0)}
TWO = ("130 bands", "130 bands, 40 dB")
# schedule, T, the largest render length reserved
A = dict(sched=([64, 256, 1024, 4096], [4, 4, 4, 4]), T=21760, max_taps=16384)     # R = 16384: two windows, the second partial
B = dict(sched=([16384], [1]), T=16384, max_taps=16384)                            # one whole window
C8 = dict(sched=([16384], [8]), T=131072, max_taps=131072)                         # R = 32768: four windows; R = T: two combine passes
ROOM = dict(sched=([16384], [64]), T=1048576, max_taps=65536)
MOST = dict(sched=([16384], [64]), T=1048576, max_taps=1048576)                    # the big FFT's largest transform, a table of its own


def _noise(seed, n, dt):
    return (np.random.default_rng(seed).standard_normal(n) / np.sqrt(n)).astype(dt)


def _convolver(hip, rs, plan, long=True, minimum=True, fmt=None):
    """one filter with a second set and a base, every reservation (the new one unless long=False)"""
    nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, 1, 1)
    assert nu.taps == plan["T"]
    if fmt:
        nu.set_interleaved(0, fmt)
        nu.set_interleaved(1, fmt)
    nu.reserve_update()
    nu.reserve_eq(plan["max_taps"])
    if minimum:
        nu.reserve_eq_minimum()
    if long:
        nu.reserve_eq_base_long()                              # in front of reserve_eq_base: the order is free
    nu.add_filter(0, 0, _noise(1, plan["T"], DT[rs]))
    assert nu.add_coeff(0, _noise(2, plan["T"], DT[rs])) == 1
    nu.reserve_eq_base(0)
    nu.finalize()
    return nu


_renderers = {}


def _renderer(hip, rs, plan_name):
    """one convolver per precision and schedule for the tests that only make synchronous calls on it"""
    if (rs, plan_name) not in _renderers:
        _renderers[(rs, plan_name)] = _convolver(hip, rs, globals()[plan_name])
    return _renderers[(rs, plan_name)]


def _bases(T, R, dt):
    full = _noise(20 + R, T, dt)
    return {"full-length noise": full, "noise with R trailing zeros": np.concatenate([full[:T - R], np.zeros(R, dt)])}


# ---------------------------------------------------------------- 1, 2: the truncated convolution

def _kernel_alone(hip, rs, plan_name, R, curves=TWO, modes=MODES):
    nu = _renderer(hip, rs, plan_name)
    T = nu.taps
    assert R > 8192
    for bname, base in _bases(T, R, DT[rs]).items():
        nu.set_eq_base(0, base)
        for name in curves:
            for mode in modes:
                e = nu.render_eq(R, *CURVES[name], mode=mode)
                got = nu.render_eq_base(0, R, *CURVES[name], mode=mode)
                assert got.dtype == DT[rs] and got.shape == (T,)
                want = eq_base_ref.apply_fft(base.astype(np.float64), e.astype(np.float64), T)
                err = cases.rel_rms(got, want)
                print("rs %d T %d R %d %s, %s, %s: rel rms %.3g (limit %g)" % (rs, T, R, bname, name, mode, err, TOL[rs]))
                # T = R: the base with R trailing zeros is all zeros, and so is the result, exactly
                assert np.any(want) == np.any(base) and err <= TOL[rs], (bname, name, mode)
                assert np.array_equal(got, nu.render_eq_base(0, R, *CURVES[name], mode=mode)), (bname, name, mode)   # same arguments, same bytes


@pytest.mark.parametrize("plan_name,R", [("A", 16384), ("B", 16384), ("C8", 32768), ("C8", 131072)])
@pytest.mark.parametrize("rs", [4, 8])
def test_long_render_onto_a_base_is_the_truncated_convolution(hip, rs, plan_name, R):
    _kernel_alone(hip, rs, plan_name, R)


def test_long_render_onto_a_base_of_the_room_correction_length(hip):
    _kernel_alone(hip, 4, "ROOM", 65536, modes=("minimum",))


def test_long_render_onto_a_base_at_the_largest_length(hip):
    """max_taps = 1 048 576 is the one reservation whose window transform (1 048 576 points) is longer than
    every table the plain render owns, and R = T is one window of it"""
    nu = _renderer(hip, 4, "MOST")
    T = R = nu.taps
    base = _noise(20, T, np.float32)
    nu.set_eq_base(0, base)
    e = nu.render_eq(R, *CURVES["130 bands, 40 dB"])
    got = nu.render_eq_base(0, R, *CURVES["130 bands, 40 dB"])
    want = eq_base_ref.apply_fft(base.astype(np.float64), e.astype(np.float64), T)
    err = cases.rel_rms(got, want)
    print("rs 4 T %d R %d: rel rms %.3g (limit %g)" % (T, R, err, TOL[4]))
    assert np.any(want) and err <= TOL[4]
    assert np.array_equal(got, nu.render_eq_base(0, R, *CURVES["130 bands, 40 dB"]))
    _renderers.pop((4, "MOST")).close()                        # 100 MB of scratch: not kept for the session


# ---------------------------------------------------------------- 3: a flat curve

@pytest.mark.parametrize("rs", [4, 8])
def test_flat_curve_gives_the_base_back_or_delays_it_by_half_its_length(hip, rs):
    nu = _renderer(hip, rs, "A")
    T, R = nu.taps, 16384
    base = _noise(30, T, DT[rs])
    nu.set_eq_base(0, base)
    b = base.astype(np.float64)
    for mode, shift in (("minimum", 0), ("linear", R // 2)):
        got = nu.render_eq_base(0, R, *CURVES["flat"], mode=mode)
        want = np.concatenate([np.zeros(shift), b[:T - shift]])
        err = cases.rel_rms(got, want)
        print("rs %d T %d R %d %s: rel rms against the base %d frames later %.3g (limit %g)" % (rs, T, R, mode, shift, err, TOL[rs]))
        assert err <= TOL[rs], mode


# ---------------------------------------------------------------- 4: the reservation alone

def _both(hip, nu, out, taps, curve, mode, coeff=1):
    L, n_bands = hip.lib(), len(curve[0])
    f, m, p = (hip._darr(list(v)) for v in curve)
    r = (L.bfhip_nupc_render_eq_base_async(nu.h, 0, coeff, taps, n_bands, f, m, p, mode),
         L.bfhip_nupc_render_eq_base(nu.h, 0, taps, n_bands, f, m, p, mode, out.ctypes.data_as(C.c_void_p)))
    assert not nu.update_busy() and not np.any(out)
    return r


@pytest.mark.parametrize("rs", [4, 8])
def test_the_reservation_alone_changes_no_byte_up_to_8192_taps(hip, rs):
    with_it, without = _renderer(hip, rs, "A"), _convolver(hip, rs, A, long=False)
    base = _noise(31, A["T"], DT[rs])
    for nu in (with_it, without):
        nu.set_eq_base(0, base)
    for R in (8192, 64):
        for mode in MODES:
            got = [nu.render_eq_base(0, R, *CURVES["130 bands"], mode=mode) for nu in (with_it, without)]
            assert np.any(got[0]) and np.array_equal(got[0], got[1]), (R, mode)
    out = np.zeros(A["T"], DT[rs])
    assert _both(hip, without, out, 16384, CURVES["130 bands"], LINEAR) == (EINVAL, EINVAL)
    assert b"8192" in hip.lib().bfhip_nupc_last_error()


# ---------------------------------------------------------------- 5: asynchronous call, set bytes and switch

@pytest.mark.parametrize("rs,mode", [(4, "minimum"), (8, "linear")])
def test_long_render_into_a_set_has_the_bits_of_the_upload_and_is_heard(hip, rs, mode):
    R, n_periods = 16384, 400
    base = _noise(13, A["T"] - R, DT[rs])                      # R trailing zeros: nothing is truncated
    x = np.random.default_rng(5).standard_normal((n_periods * 64, 1)) * 0.02
    raws, news = [], []
    for how in ("base", "upload"):
        nu = _convolver(hip, rs, A, fmt="FLOAT64_LE")
        assert nu.L0 == 64
        nu.set_eq_base(0, base)
        new = nu.render_eq_base(0, R, *CURVES["130 bands"], mode=mode)
        if how == "base":
            nu.render_eq_base_async(0, 1, R, *CURVES["130 bands"], mode=mode)
        else:
            nu.update_coeff_async(0, 1, new)
        assert nu.update_wait() == 0
        nu.set_crossfade(0)
        nu.set_coeff(0, 1)
        raws.append(np.concatenate([nu.block(x[p * 64:(p + 1) * 64])[1] for p in range(n_periods)]))
        news.append(new)
        t_sw = nu.switch_frame()
    assert np.array_equal(news[0], news[1]) and np.any(news[0])
    assert np.array_equal(raws[0], raws[1])
    fmts = [nupc_ref.fmt("FLOAT64_LE")]
    got = nupc_ref.decode(raws[0], fmts, len(x))[:, 0]
    want = nupc_ref.conv(x[:, 0], news[0].astype(np.float64), len(x))
    assert 0 <= t_sw and t_sw + R <= len(x), "the run must go on for the curve's length beyond the switch"
    err = cases.rel_rms(got[t_sw:], want[t_sw:])
    print("rs %d %s: switch at frame %d, rel rms from there on %.3g (limit %g)" % (rs, mode, t_sw, err, TOL[rs]))
    assert err <= TOL[rs]
    old = nupc_ref.conv(x[:, 0], _noise(1, A["T"], DT[rs]).astype(np.float64), len(x))
    assert cases.rel_rms(got[t_sw:], old[t_sw:]) > 0.5                      # and not the old set's


# ---------------------------------------------------------------- 6: errors change nothing

def test_argument_and_state_errors_change_nothing(hip):
    L = hip.lib()
    good = CURVES["130 bands"]
    nu = hip.Nupc(*A["sched"], 4, 1, 1)
    nu.reserve_update()
    assert L.bfhip_nupc_reserve_eq_base_long(nu.h) == ESTATE                # before reserve_eq
    assert b"reserve_eq" in L.bfhip_nupc_last_error()
    nu.reserve_eq(16384)
    nu.add_filter(0, 0, _noise(1, A["T"], np.float32))
    assert nu.add_coeff(0, _noise(2, A["T"], np.float32)) == 1
    nu.reserve_eq_base(0)
    nu.reserve_eq_base_long()                                               # behind reserve_eq_base this time
    nu.finalize()
    assert L.bfhip_nupc_reserve_eq_base_long(nu.h) == ESTATE                # after finalize
    before = nu.render_eq_base(0, 16384, *good)
    out = np.zeros(nu.taps, np.float32)
    for taps in (32768, 0, 12, 24576):                                      # above max_taps, not a power of two >= 8
        assert _both(hip, nu, out, taps, good, LINEAR) == (EINVAL, EINVAL), taps
        assert b"16384" in L.bfhip_nupc_last_error()                        # the limit in force
    assert _both(hip, nu, out, 16384, good, MINIMUM) == (ESTATE, ESTATE)     # no reserve_eq_minimum
    assert b"reserve_eq_minimum" in L.bfhip_nupc_last_error()
    assert nu.update_result() == 0
    assert np.any(before) and np.array_equal(nu.render_eq_base(0, 16384, *good), before)
    # with every reservation: minimum mode has the same limit
    nu = _renderer(hip, 4, "A")
    before = nu.render_eq_base(0, 16384, *good, mode="minimum")
    for mode in (LINEAR, MINIMUM):
        assert _both(hip, nu, out, 32768, good, mode) == (EINVAL, EINVAL), mode
        assert b"16384" in L.bfhip_nupc_last_error()
    assert np.any(before) and np.array_equal(nu.render_eq_base(0, 16384, *good, mode="minimum"), before)
