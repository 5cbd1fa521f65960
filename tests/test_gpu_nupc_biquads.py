"""GPU: parametric-equaliser sections rendered on the device (bfhip_nupc_render_biquads*,
include/bfhip_nupc.h; brutefir_amd/csrc/eq_biquad.h).

What must hold: the render alone is the float64 model's (tests/biquad_ref.py) at the project's parity bars,
float32 1e-5 / float64 1e-12 relative RMS, in both phases, for the five shared section sets, on the
one-workgroup path (R <= 16384) and on the big-FFT sequence with each combine radix and with two passes;
a render is a pure function of its arguments; render_biquads_async into an idle set followed by a switch
has the BYTES of update_coeff_async with the array render_biquads returned, and the output behind the switch
is the float64 model's (tests/nupc_ref.py); a flat cascade passes the input (OWN) or delays it by R/2 frames
(LINEAR); onto a base the result is the truncated convolution of the model's taps with the base
(tests/eq_base_ref.py); a group yields the bytes of the single calls; nothing else moves; and every argument
and state error answers its code and changes nothing.

Why the bars have room: both sides evaluate the same float64 form.  Perturbing every sine of the model by
+-2 ulp moves the taps by 2e-16 (`room`) to 4e-15 (`many`) relative RMS; rounding X to float32 by 2e-8 .. 3e-8."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import biquad_ref
import cases
import eq_base_ref
import eq_ref
import nupc_ref

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
DT = {4: np.float32, 8: np.float64}
EINVAL, ESTATE = -1, -5
SETS = biquad_ref.sets()
PHASES = ["own", "linear"]
LENGTHS = [8, 64, 4096, 16384, 32768, 65536, 131072, 262144]
# schedule, blocks run, block the render starts before, block the switch is requested before, render length
SMALL = dict(sched=([16, 32, 64], [2, 2, 4]), n_blocks=60, b_render=3, b_switch=12, R=256)
BIG = dict(sched=([64, 256, 1024, 4096, 16384], [4, 4, 4, 4, 1]), n_blocks=1300, b_render=3, b_switch=40, R=32768)


def _noise(seed, n, dt):
    return (np.random.default_rng(seed).standard_normal(n) / np.sqrt(n)).astype(dt)


@functools.lru_cache(maxsize=None)
def _model(R, name, phase):
    taps = biquad_ref.render(R, SETS[name], phase)
    taps.setflags(write=False)
    return taps


_renderers = {}


def _make_renderer(hip, rs):
    """the renderer of tests/test_gpu_nupc_eq.py: a single 16384-frame segment, 1 048 576 taps in float32 and
    262 144 in float64, one filter with a second set to render into"""
    nu = hip.Nupc([16384], [64 if rs == 4 else 16], rs, 1, 1)
    nu.reserve_update()
    nu.reserve_eq(nu.taps)
    nu.add_filter(0, 0, _noise(1, 64, DT[rs]))
    assert nu.add_coeff(0, _noise(2, 64, DT[rs])) == 1
    nu.finalize()
    return nu


@pytest.fixture(scope="module", autouse=True)
def _leave_no_convolver_behind():
    """the shared renderers are closed, and the runs' convolvers collected, before the next file starts: its
    timing-sensitive tests then meet no destructor of this file's"""
    yield
    for nu in _renderers.values():
        nu.close()
    _renderers.clear()
    gc.collect()


def _renderer(hip, rs):
    if rs not in _renderers:
        _renderers[rs] = _make_renderer(hip, rs)
    return _renderers[rs]


# ---------------------------------------------------------------- 1: the render alone

@pytest.mark.parametrize("R", LENGTHS)
@pytest.mark.parametrize("rs", [4, 8])
def test_render_is_the_float64_model(hip, rs, R):
    nu = _renderer(hip, rs)
    for phase in PHASES:
        for name, sections in SETS.items():
            got = nu.render_biquads(R, sections, phase)
            assert got.dtype == DT[rs] and got.shape == (R,)
            err = cases.rel_rms(got, _model(R, name, phase))
            print("rs %d R %d %s %s: rel rms %.3g (limit %g)" % (rs, R, name, phase, err, TOL[rs]))
            assert err <= TOL[rs], (name, phase)
            assert np.array_equal(got, nu.render_biquads(R, sections, phase)), (name, phase)   # a pure function


@pytest.mark.parametrize("phase", PHASES)
def test_render_of_the_full_room_correction_length(hip, phase):
    nu, R = _renderer(hip, 4), 1048576
    got = nu.render_biquads(R, SETS["room"], phase)
    err = cases.rel_rms(got, _model(R, "room", phase))
    print("rs 4 R %d room %s: rel rms %.3g (limit %g)" % (R, phase, err, TOL[4]))
    assert err <= TOL[4]
    assert np.array_equal(got, nu.render_biquads(R, SETS["room"], phase))


# ---------------------------------------------------------------- runs with a switch onto a rendered set

class Run:
    """one filter with two sets of flat noise; `how` rewrites set 1 before block b_render: "biquads"
    render_biquads_async, "upload" update_coeff_async with the array render_biquads returns, None not at all;
    the switch 0 -> 1 is requested before block b_switch"""

    def __init__(self, hip, rs, plan, out_fmt, how, name="tone", phase="own", wait_at_switch=False, switch=True):
        dt = DT[rs]
        self.nu = nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, 1, 1)
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, out_fmt)
        nu.reserve_update()
        nu.reserve_eq(plan["R"])
        self.h = [_noise(11, nu.taps, dt), _noise(12, nu.taps, dt)]
        nu.add_filter(0, 0, self.h[0])
        assert nu.add_coeff(0, self.h[1]) == 1
        nu.finalize()
        self.L0, R = nu.L0, plan["R"]
        self.x = (np.random.default_rng(5).standard_normal((plan["n_blocks"] * nu.L0, 1)) * 0.02).astype(dt)
        got = []
        for b in range(plan["n_blocks"]):
            if b == plan["b_render"] and how == "biquads":
                nu.render_biquads_async(0, 1, R, SETS[name], phase)
                if not wait_at_switch:
                    assert nu.update_wait() == 0
            if b == plan["b_render"] and how == "upload":
                nu.update_coeff_async(0, 1, nu.render_biquads(R, SETS[name], phase))
                assert nu.update_wait() == 0
            if b == plan["b_switch"] and switch:
                if how == "biquads" and wait_at_switch:
                    assert nu.update_wait() == 0
                nu.set_coeff(0, 1)
            got.append(nu.block(self.x[b * nu.L0:(b + 1) * nu.L0]))
        self.status = [s for s, _ in got]
        self.raw = np.concatenate([r for _, r in got])
        self.t_sw = nu.switch_frame()


# ---------------------------------------------------------------- 2: into a set

@pytest.mark.parametrize("rs,plan,out_fmt,name,phase", [(4, SMALL, "S24_4LE", "tone", "own"), (4, SMALL, "S24_4LE", "many", "linear"),
                                                        (8, BIG, "FLOAT64_LE", "room", "own")],
                         ids=["f32 lds own", "f32 lds linear", "f64 big own"])
def test_render_into_a_set_has_the_bits_of_the_upload(hip, rs, plan, out_fmt, name, phase):
    a = Run(hip, rs, plan, out_fmt, "biquads", name, phase)
    b = Run(hip, rs, plan, out_fmt, "upload", name, phase)
    assert a.nu.taps >= plan["R"] and a.t_sw == b.t_sw and a.t_sw > 0
    assert (a.t_sw + a.L0 + a.nu.taps) < len(a.x), "the run must go on beyond the switch window"
    assert a.status == b.status
    assert np.array_equal(a.raw, b.raw)
    assert np.any(a.raw[(a.t_sw + a.L0) * a.nu.out_bytes // a.L0:])


def _decoded(r, rs):
    fmts = [nupc_ref.fmt(FF[rs])]
    return fmts, nupc_ref.decode(r.raw, fmts, len(r.x))


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("rs", [4, 8])
def test_output_after_the_switch_is_the_models(hip, rs, phase):
    r = Run(hip, rs, SMALL, FF[rs], "biquads", "mixed", phase)
    L0, n = r.L0, len(r.x)
    eq = np.concatenate([_model(SMALL["R"], "mixed", phase), np.zeros(r.nu.taps - SMALL["R"])])
    x = r.x.astype(np.float64)
    ys = [nupc_ref.convolve(x, [(0, 0, h, 1.0, 1.0)], 1) for h in (r.h[0], eq)]
    want = nupc_ref.switched(ys, [(r.t_sw, L0, 1)])
    fmts, got = _decoded(r, rs)
    want = nupc_ref.decode(nupc_ref.encode(want, fmts, L0)[0], fmts, n)
    err = cases.rel_rms(got, want)
    print("rs %d %s: rel rms whole run %.3g (limit %g)" % (rs, phase, err, TOL[rs]))
    assert err <= TOL[rs]
    t = r.t_sw + L0                                # behind the fade: the rendered set alone
    assert t < n - L0 and cases.rel_rms(got[t:], ys[1][t:]) <= TOL[rs]


@pytest.mark.parametrize("rs", [4, 8])
def test_a_flat_cascade_passes_or_delays_the_input(hip, rs):
    R = SMALL["R"]
    for phase, delay in (("own", 0), ("linear", R // 2)):
        r = Run(hip, rs, SMALL, FF[rs], "biquads", "flat", phase)
        _, got = _decoded(r, rs)
        t, n = r.t_sw + r.L0, len(r.x)
        assert 0 < r.t_sw and t + R < n
        x = r.x.astype(np.float64)
        err = cases.rel_rms(got[t:], x[t - delay:n - delay])
        print("rs %d flat %s: rel rms %.3g (limit %g)" % (rs, phase, err, TOL[rs]))
        assert err <= TOL[rs], phase


# ---------------------------------------------------------------- 3: onto a base and in a group

def _base_convolver(hip, rs, long):
    """one 16384-frame segment of two partitions, T = 32768; filter 0 has a base of full-length noise"""
    nu = hip.Nupc([16384], [2], rs, 1, 1)
    nu.reserve_update()
    nu.reserve_eq(nu.taps)
    if long:
        nu.reserve_eq_base_long()
    nu.add_filter(0, 0, _noise(21, nu.taps, DT[rs]))
    assert nu.add_coeff(0, _noise(22, nu.taps, DT[rs])) == 1
    nu.reserve_eq_base(0)
    nu.finalize()
    return nu


@pytest.mark.parametrize("long", [False, True], ids=["lds windows", "long windows"])
@pytest.mark.parametrize("rs", [4, 8])
def test_render_onto_a_base_is_the_truncated_convolution(hip, rs, long):
    nu = _base_convolver(hip, rs, long)
    T = nu.taps
    base = _noise(21, T, DT[rs])                   # what add_filter gave the base at finalize
    for eq_taps, name, phase in ([(32768, "room", "own"), (32768, "tone", "linear")] if long else
                                 [(64, "mixed", "own"), (64, "tone", "linear"), (8192, "room", "own"), (8192, "many", "linear")]):
        got = nu.render_biquads_base(0, eq_taps, SETS[name], phase)
        assert got.dtype == DT[rs] and got.shape == (T,)
        want = eq_base_ref.apply_fft(base, _model(eq_taps, name, phase), T)
        err = cases.rel_rms(got, want)
        print("rs %d eq_taps %d %s %s: rel rms %.3g (limit %g)" % (rs, eq_taps, name, phase, err, TOL[rs]))
        assert err <= TOL[rs], (eq_taps, name, phase)
        assert np.array_equal(got, nu.render_biquads_base(0, eq_taps, SETS[name], phase))
    if not long:
        assert hip.lib().bfhip_nupc_render_biquads_base_async(nu.h, 0, 1, 16384, 1, hip._darr([1.0, 0, 0, 0, 0]), 0) == EINVAL
        assert b"8192" in hip.lib().bfhip_nupc_last_error()
    nu.close()


GROUP = [(0, 1, 1), (1, 1, 0), (2, 1, 1)]           # (filter, set, onto its base): two onto their bases, one plain


def _crossbar(hip, rs, plan, group):
    """1 input, 3 outputs: filter f feeds output f; two sets each; filters 0 and 2 have bases"""
    nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, 1, 3)
    nu.set_interleaved(0, FF[rs])
    nu.set_interleaved(1, FF[rs])
    nu.reserve_update()
    nu.reserve_eq(64)
    if group:
        nu.reserve_eq_group(group)
    for f in range(3):
        nu.add_filter(0, f, _noise(100 + f, nu.taps, DT[rs]))
        assert nu.add_coeff(f, _noise(200 + f, nu.taps, DT[rs])) == 1
    for f in (0, 2):
        nu.reserve_eq_base(f)
    nu.finalize()
    return nu


def _crossbar_run(nu, plan, render, switch=True):
    x = (np.random.default_rng(5).standard_normal((plan["n_blocks"] * nu.L0, 1)) * 0.02).astype(nu.dt)
    got = []
    for b in range(plan["n_blocks"]):
        if b == plan["b_render"]:
            render(nu)
        if b == plan["b_switch"] and switch:
            for f, c, _ in GROUP:
                nu.set_coeff(f, c)
        got.append(nu.block(x[b * nu.L0:(b + 1) * nu.L0])[1])
    return np.concatenate(got)


def _singles(name, phase, upload=False):
    def go(nu):
        for f, c, onto in GROUP:
            if upload:
                taps = nu.render_biquads_base(f, 64, SETS[name], phase) if onto else nu.render_biquads(64, SETS[name], phase)
                nu.update_coeff_async(f, c, taps)
            elif onto:
                nu.render_biquads_base_async(f, c, 64, SETS[name], phase)
            else:
                nu.render_biquads_async(f, c, 64, SETS[name], phase)
            assert nu.update_wait() == 0
    return go


def _group(hip, name, phase):
    def go(nu):
        nu.render_biquads_group_async([m[0] for m in GROUP], [m[1] for m in GROUP], [m[2] for m in GROUP], 64, SETS[name], phase)
        assert nu.update_wait() == 0
        for i in range(len(GROUP)):
            assert nu.update_result_member(i) == 0
        assert hip.lib().bfhip_nupc_update_result_member(nu.h, len(GROUP)) == EINVAL      # the group had three members
    return go


@pytest.mark.parametrize("rs,name,phase", [(4, "mixed", "own"), (8, "tone", "linear")])
def test_group_and_base_calls_have_the_bytes_of_the_upload(hip, rs, name, phase):
    """a group of three (two onto their bases, one plain), the three single calls, and the uploads of the three
    synchronous calls' arrays: the same output bytes behind the switch"""
    runs = []
    for group, render in ((3, _group(hip, name, phase)), (0, _singles(name, phase)), (0, _singles(name, phase, upload=True))):
        nu = _crossbar(hip, rs, SMALL, group)
        runs.append(_crossbar_run(nu, SMALL, render))
        assert nu.switch_frame() > 0
        nu.close()
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[1], runs[2])
    assert np.any(runs[0][-3 * 16 * rs:])


# ---------------------------------------------------------------- 4: nothing else moves

@pytest.mark.parametrize("rs,plan", [(4, SMALL), (8, BIG)], ids=["f32 lds", "f64 big"])
def test_render_into_an_idle_set_changes_no_byte_before_the_switch(hip, rs, plan):
    plan = dict(plan, n_blocks=plan["b_switch"] + 20)
    a = Run(hip, rs, plan, FF[rs], "biquads", "room", wait_at_switch=True, switch=False)     # rendered, never switched to
    b = Run(hip, rs, plan, FF[rs], None, switch=False)
    assert a.nu.update_wait() == 0
    assert np.array_equal(a.raw, b.raw)
    a = Run(hip, rs, plan, FF[rs], "biquads", "room", wait_at_switch=True)                   # the render beside the periods
    b = Run(hip, rs, plan, FF[rs], None)
    cut = a.t_sw // a.L0 * a.nu.out_bytes
    assert a.t_sw == b.t_sw and cut > 0 and np.array_equal(a.raw[:cut], b.raw[:cut])


@pytest.mark.parametrize("rs", [4, 8])
def test_band_renders_keep_their_bytes_around_a_section_render(hip, rs):
    nu = _renderer(hip, rs)
    curve = eq_ref.random_bands(130, 7)
    for R in (4096, 65536):
        before = nu.render_eq(R, *curve)
        assert np.any(nu.render_biquads(R, SETS["many"], "linear"))
        assert np.array_equal(nu.render_eq(R, *curve), before)
        assert cases.rel_rms(before, eq_ref.render(R, *curve)) <= TOL[rs]


# ---------------------------------------------------------------- 5: errors

def _bad_sections():
    good = SETS["tone"]
    nan = float("nan")

    def with_(k, i, v):
        s = np.array(good)
        s[k, i] = v
        return s
    return {"0 sections": np.zeros((0, 5)), "33 sections": np.tile(SETS["flat"], (33, 1)), "NaN b1": with_(1, 1, nan),
            "Inf a1": with_(2, 3, float("inf")), "a2 = 1": with_(0, 4, 1.0), "a2 = -1": with_(0, 4, -1.0),
            "a1 = 1 + a2": with_(1, 3, 1.0 + good[1, 4]), "a1 = -(1 + a2)": with_(1, 3, -(1.0 + good[1, 4]))}


def _sec(hip, s):
    s = np.ascontiguousarray(s, np.float64)
    return len(s), hip._darr(list(s.ravel()))


def test_argument_and_state_errors_change_nothing(hip):
    L = hip.lib()
    plan = SMALL
    twin = _crossbar_run(_crossbar(hip, 4, plan, 3), plan, _group(hip, "tone", "own"))
    nu = _crossbar(hip, 4, plan, 3)                       # reserve_eq(64): max_taps 64, bases on filters 0 and 2
    h = nu.h
    out = np.zeros(nu.taps, np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    three = lambda v: (C.c_int * 3)(*v)
    F, S, B = three([0, 1, 2]), three([1, 1, 1]), three([1, 0, 1])

    def every(taps, sections, phase=0):
        n, p = _sec(hip, sections)
        r = (L.bfhip_nupc_render_biquads(h, taps, n, p, phase, po),
             L.bfhip_nupc_render_biquads_async(h, 1, 1, taps, n, p, phase),
             L.bfhip_nupc_render_biquads_base(h, 0, taps, n, p, phase, po),
             L.bfhip_nupc_render_biquads_base_async(h, 0, 1, taps, n, p, phase),
             L.bfhip_nupc_render_biquads_group_async(h, 3, F, S, B, taps, n, p, phase))
        assert not nu.update_busy() and not np.any(out)
        return r

    for name, s in _bad_sections().items():
        assert every(64, s) == (EINVAL,) * 5, name
        if "sections" not in name:
            assert b"section " in L.bfhip_nupc_last_error(), name
    for phase in (2, -1):
        assert every(64, SETS["tone"], phase) == (EINVAL,) * 5, phase
    for taps in (0, 4, 48, 63, 128, -64):                 # not a power of two, below 8, above max_taps / the limit in force
        assert every(taps, SETS["tone"]) == (EINVAL,) * 5, taps
    n, p = _sec(hip, SETS["tone"])
    assert L.bfhip_nupc_render_biquads(h, 64, n, None, 0, po) == EINVAL
    assert L.bfhip_nupc_render_biquads(h, 64, n, p, 0, None) == EINVAL
    assert L.bfhip_nupc_render_biquads_async(h, 3, 1, 64, n, p, 0) == EINVAL          # no such filter
    assert L.bfhip_nupc_render_biquads_async(h, 0, 2, 64, n, p, 0) == EINVAL          # no such set
    assert L.bfhip_nupc_render_biquads_async(h, 0, 0, 64, n, p, 0) == ESTATE          # live
    assert L.bfhip_nupc_render_biquads_base_async(h, 0, 0, 64, n, p, 0) == ESTATE     # live
    assert L.bfhip_nupc_render_biquads_base_async(h, 1, 1, 64, n, p, 0) == ESTATE     # no base reservation
    assert b"reserve_eq_base" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_render_biquads_base(h, 1, 64, n, p, 0, po) == ESTATE
    assert L.bfhip_nupc_render_biquads_base_async(h, -1, 1, 64, n, p, 0) == EINVAL
    # a bad member: no member is touched
    assert L.bfhip_nupc_render_biquads_group_async(h, 3, F, three([1, 1, 0]), B, 64, n, p, 0) == ESTATE      # member 2 is live
    assert b"member 2" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_render_biquads_group_async(h, 3, F, S, three([1, 1, 1]), 64, n, p, 0) == ESTATE      # member 1 has no base
    assert b"member 1" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_render_biquads_group_async(h, 3, three([0, 1, 1]), S, three([1, 0, 0]), 64, n, p, 0) == EINVAL   # the same set twice
    assert L.bfhip_nupc_render_biquads_group_async(h, 4, F, S, B, 64, n, p, 0) == EINVAL
    assert L.bfhip_nupc_render_biquads_group_async(h, 0, F, S, B, 64, n, p, 0) == EINVAL
    assert not nu.update_busy() and nu.update_result() == 0 and not np.any(out)
    # after all of them the convolver does what its twin does, which made none of these calls
    assert np.array_equal(_crossbar_run(nu, plan, _group(hip, "tone", "own")), twin)
    # and the sets it switched to are live now: a queued switch back makes set 0 busy as well
    nu.set_coeff(0, 0)
    assert L.bfhip_nupc_render_biquads_async(h, 0, 0, 64, n, p, 0) == ESTATE          # queued
    assert L.bfhip_nupc_render_biquads_async(h, 0, 1, 64, n, p, 0) == ESTATE          # live
    assert L.bfhip_nupc_render_biquads_group_async(h, 1, three([0, 0, 0]), three([0, 0, 0]), None, 64, n, p, 0) == ESTATE


def test_without_the_reservations(hip):
    L = hip.lib()
    n, p = _sec(hip, SETS["tone"])
    out = np.zeros(512, np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    one = (C.c_int * 1)(0)
    set1 = (C.c_int * 1)(1)
    for reserve_eq in (False, True):
        nu = hip.Nupc(*SMALL["sched"], 4, 1, 1)
        nu.reserve_update()
        if reserve_eq:
            nu.reserve_eq(64)
        nu.add_filter(0, 0, _noise(1, nu.taps, np.float32))
        assert nu.add_coeff(0, _noise(2, nu.taps, np.float32)) == 1
        nu.finalize()
        h = nu.h
        if not reserve_eq:
            assert L.bfhip_nupc_render_biquads_async(h, 0, 1, 64, n, p, 0) == ESTATE
            assert b"reserve_eq" in L.bfhip_nupc_last_error()
            assert L.bfhip_nupc_render_biquads(h, 64, n, p, 0, po) == ESTATE
        assert L.bfhip_nupc_render_biquads_base_async(h, 0, 1, 64, n, p, 0) == ESTATE
        assert L.bfhip_nupc_render_biquads_base(h, 0, 64, n, p, 0, po) == ESTATE
        assert L.bfhip_nupc_render_biquads_group_async(h, 1, one, set1, None, 64, n, p, 0) == ESTATE
        assert not nu.update_busy() and not np.any(out)
        nu.update_coeff_async(0, 1, _noise(3, nu.taps, np.float32))            # the rewrite itself is as before
        assert nu.update_wait() == 0
        nu.close()


def test_calls_while_a_render_is_in_flight(hip):
    """1 048 576 taps into 64 partitions of 16384: the host calls below take microseconds, the device work does
    not; that the rewrite was still in flight behind the last of them is asserted"""
    L = hip.lib()
    nu = _make_renderer(hip, 4)
    h, R = nu.h, nu.taps
    out = np.zeros(R, np.float32)
    n, p = _sec(hip, SETS["room"])
    freq, mag, phase = (hip._darr(v) for v in eq_ref.flat())
    # a new convolver's first rewrite spends milliseconds inside the call (streams and kernels used for the
    # first time), longer than the device work takes: that one is made and waited for beforehand
    nu.render_biquads_async(0, 1, R, SETS["many"], "linear")
    assert nu.update_wait() == 0 and not nu.update_busy()
    nu.render_biquads_async(0, 1, R, SETS["room"], "own")
    answers = [L.bfhip_nupc_set_coeff(h, 0, 1),
               L.bfhip_nupc_render_biquads_async(h, 0, 1, R, n, p, 0),
               L.bfhip_nupc_render_eq_async(h, 0, 1, R, 2, freq, mag, phase),
               L.bfhip_nupc_render_biquads(h, 8, n, p, 0, out.ctypes.data_as(C.c_void_p))]
    assert nu.update_busy(), "the rewrite was over before the calls were made: nothing was tested"
    assert answers == [ESTATE] * 4
    assert nu.update_wait() == 0 and nu.update_result() == 0 and not nu.update_busy() and not np.any(out)
    # the set holds the render: a pulse through it, hard switch at frame 0, is the model's first taps
    nu.set_crossfade(0)
    nu.set_coeff(0, 1)
    x = np.zeros((nu.L0, 1), np.float32)
    x[0] = 1.0
    y = np.frombuffer(nu.block(x)[1].tobytes(), np.float32)
    assert nu.switch_frame() == 0
    assert cases.rel_rms(y, _model(R, "room", "own")[:nu.L0]) <= TOL[4]
    nu.close()
