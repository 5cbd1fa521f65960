"""GPU: one equaliser render across a group of filters (bfhip_nupc_reserve_eq_group / _render_eq_group_async /
_update_result_member, include/bfhip_nupc.h; the batched window kernel of brutefir_amd/csrc/eq_apply.h).

Every comparison is byte equality: against a twin convolver that makes the same renders with the single calls
(render_eq_base_async / render_eq_async, update_wait between them), which tests/test_gpu_nupc_eq_base.py and
its neighbours hold to the float64 models, or against a twin that renders nothing.  What must hold: a group of
1, 2, 4 = max_members and 16 members leaves in every member's set the bytes of its single call, at float32 and
float64, in both modes, on the plans of the eq-base tests and on one long curve through the big FFT; a group
in flight changes no byte of the sets that are live, in both switch modes; a failing check on any member
changes nothing for any member; every call made while a group is in flight answers BFHIP_ESTATE and works
afterwards; a member that ends non-finite is reported alone and stays locked alone; the call is pure."""
import ctypes as C

import numpy as np
import pytest

import eq_base_ref
import eq_ref

pytestmark = pytest.mark.gpu
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
DT = {4: np.float32, 8: np.float64}
EINVAL, ESTATE = -1, -5
LINEAR, MINIMUM = 0, 1
CURVE = eq_ref.random_bands(130, 7)
# schedule, render length, blocks run, block the render starts before, block the switch is requested before
PLANS = {
    "S48 R8": dict(sched=([8, 16], [2, 2]), R=8, n_blocks=30, b_render=3, b_switch=8),
    "S48 R32": dict(sched=([8, 16], [2, 2]), R=32, n_blocks=30, b_render=3, b_switch=8),
    "SMALL": dict(sched=([16, 32, 64], [2, 2, 4]), R=256, n_blocks=60, b_render=3, b_switch=12),
    "MID": dict(sched=([32, 128, 512], [4, 4, 4]), R=1024, n_blocks=130, b_render=3, b_switch=12),     # two background segments
    "LONG": dict(sched=([16384], [1]), R=16384, n_blocks=5, b_render=1, b_switch=2, long=True),        # through the big FFT
}
BIG = dict(sched=([16384], [64]), R=8192)                       # 1 048 576 taps: a rewrite stays in flight behind its call
# (filter, set, onto its base) on the 2x2 crossbar: filters 0 and 2 have bases
GROUPS = {1: [(2, 1, 1)], 2: [(0, 1, 1), (1, 1, 0)], 4: [(0, 1, 1), (1, 1, 0), (2, 1, 1), (3, 1, 0)]}


def _noise(seed, n, dt):
    return (np.random.default_rng(seed).standard_normal(n) / np.sqrt(n)).astype(dt)


def _convolver(hip, rs, plan, side=2, group=4, base_filters=(0, 2), bases=None, mode=None, fmt=None):
    """side x side crossbar, filter f = side * in + out, three sets each (0 live), full-length noise bases (the
    truncation at T cuts their tails)"""
    dt = DT[rs]
    nu = hip.Nupc(plan["sched"][0], plan["sched"][1], rs, side, side)
    nu.set_interleaved(0, FF[rs])
    nu.set_interleaved(1, fmt or FF[rs])
    nu.reserve_update()
    nu.reserve_eq(plan["R"])
    nu.reserve_eq_minimum()
    if plan.get("long"):
        nu.reserve_eq_base_long()
    if group:
        nu.reserve_eq_group(group)
    T = nu.taps
    for f in range(side * side):
        nu.add_filter(f // side, f % side, _noise(100 + f, T, dt))
        assert nu.add_coeff(f, _noise(200 + f, T, dt)) == 1
        assert nu.add_coeff(f, _noise(300 + f, T, dt)) == 2
    for f in base_filters:
        nu.reserve_eq_base(f)
    nu.finalize()
    if mode is not None:
        nu.set_switch_mode(mode)
    for f in base_filters:
        nu.set_eq_base(f, bases[f] if bases else _noise(400 + f, T, dt))
    return nu


def _input(plan, nu, side=2):
    return (np.random.default_rng(5).standard_normal((plan["n_blocks"] * nu.L0, side)) * 0.02).astype(nu.dt)


def _run(nu, plan, x, at):
    """the blocks of x through nu; at[b](nu) is called before block b.  -> status list, raw bytes per block"""
    got = []
    for b in range(plan["n_blocks"]):
        if b in at:
            at[b](nu)
        got.append(nu.block(x[b * nu.L0:(b + 1) * nu.L0]))
    return [s for s, _ in got], [r for _, r in got]


def _group(members, R, mode, wait=True, times=1):
    def go(nu):
        for _ in range(times):
            nu.render_eq_group_async([m[0] for m in members], [m[1] for m in members], [m[2] for m in members], R, *CURVE, mode=mode)
            if wait:
                assert nu.update_wait() == 0
                for i in range(len(members)):
                    assert nu.update_result_member(i) == 0
    return go


def _singles(members, R, mode):
    def go(nu):
        for f, c, onto in members:
            if onto:
                nu.render_eq_base_async(f, c, R, *CURVE, mode=mode)
            else:
                nu.render_eq_async(f, c, R, *CURVE, mode=mode)
            assert nu.update_wait() == 0
    return go


def _switch(members, wait=False):
    def go(nu):
        if wait:
            assert nu.update_wait() == 0
        for f, c, _ in members:
            nu.set_coeff(f, c)
    return go


def _same_bytes(a, b):
    assert a[0] == b[0]
    assert len(a[1]) == len(b[1])
    for i, (u, v) in enumerate(zip(a[1], b[1])):
        assert np.array_equal(u, v), "block %d" % i


# ---------------------------------------------------------------- 1: bytes against the single calls

def _against_the_singles(hip, rs, plan, members, mode, side=2, group=4, base_filters=(0, 2), bases=None):
    x = None
    runs = []
    for grp, render in ((group, _group(members, plan["R"], mode)), (0, _singles(members, plan["R"], mode))):
        nu = _convolver(hip, rs, plan, side=side, group=grp, base_filters=base_filters, bases=bases)
        x = _input(plan, nu, side) if x is None else x
        runs.append(_run(nu, plan, x, {plan["b_render"]: render, plan["b_switch"]: _switch(members)}))
        assert nu.switch_frame() > 0
        nu.close()
    _same_bytes(*runs)
    assert np.any(runs[0][1][-1])
    return runs[0]


@pytest.mark.parametrize("size", [1, 2, 4])
@pytest.mark.parametrize("mode", ["linear", "minimum"])
@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("plan_name", list(PLANS))
def test_group_has_the_bytes_of_the_single_calls(hip, plan_name, rs, mode, size):
    _against_the_singles(hip, rs, PLANS[plan_name], GROUPS[size], mode)


@pytest.mark.parametrize("plan_name,rs,mode", [("SMALL", 4, "minimum"), ("S48 R32", 8, "linear")])
def test_group_of_sixteen_filters(hip, plan_name, rs, mode):
    members = [(f, 1 + f % 2, int(f % 3 != 1)) for f in range(16)]
    _against_the_singles(hip, rs, PLANS[plan_name], members, mode, side=4, group=16,
                         base_filters=[f for f, _, onto in members if onto])


@pytest.mark.parametrize("rs,mode", [(4, "linear"), (8, "minimum")])
def test_all_members_onto_bases_two_of_them_equal(hip, rs, mode):
    plan = PLANS["SMALL"]
    T = 352
    bases = {f: _noise(400 + f, T, DT[rs]) for f in range(4)}    # full length: the truncation cuts their tails
    bases[1] = bases[0].copy()
    members = [(f, 1, 1) for f in range(4)]
    got = _against_the_singles(hip, rs, plan, members, mode, base_filters=(0, 1, 2, 3), bases=bases)
    # and the same run with filter 1 on a base of its own differs: the members did not share a result
    bases[1] = _noise(999, T, DT[rs])
    nu = _convolver(hip, rs, plan, base_filters=(0, 1, 2, 3), bases=bases)
    other = _run(nu, plan, _input(plan, nu), {plan["b_render"]: _group(members, plan["R"], mode), plan["b_switch"]: _switch(members)})
    assert not np.array_equal(np.concatenate(other[1]), np.concatenate(got[1]))


# ---------------------------------------------------------------- 2: idle sets change no byte

@pytest.mark.parametrize("mode_name", ["SWITCH_ALIGNED", "SWITCH_STAGGERED"])
@pytest.mark.parametrize("rs,plan_name", [(4, "SMALL"), (8, "MID")])
def test_group_in_flight_changes_no_byte_of_the_live_sets(hip, rs, plan_name, mode_name):
    """a switch 0 -> 2 of every filter is committed before block 1; the group goes into sets 1 before block 3,
    while that switch is being carried out, is not waited for and is never switched to"""
    plan, members = PLANS[plan_name], GROUPS[4]
    to_2 = _switch([(f, 2, 0) for f in range(4)])
    runs = []
    for render in (_group(members, plan["R"], "minimum", wait=False), lambda nu: None):
        nu = _convolver(hip, rs, plan, mode=getattr(hip, mode_name))
        runs.append(_run(nu, plan, _input(plan, nu), {1: to_2, 3: render}))
        assert nu.update_wait() == 0 and nu.switch_frame() > 0
    _same_bytes(*runs)


# ---------------------------------------------------------------- 3: all or nothing

def _prepared(hip, nu, members, R, curve=CURVE, mode=LINEAR, n_members=None):
    """the group call with its arguments converted beforehand: calling it costs one foreign call"""
    arr = lambda v: (C.c_int * max(len(v), 1))(*v)
    f, m, p = (hip._darr(list(v)) for v in curve)
    args = (nu.h, len(members) if n_members is None else n_members, arr([v[0] for v in members]), arr([v[1] for v in members]),
            arr([v[2] for v in members]), R, len(curve[0]), f, m, p, mode)
    fn = hip.lib().bfhip_nupc_render_eq_group_async
    return lambda: fn(*args)


def _call(hip, nu, members, R, **kw):
    r = _prepared(hip, nu, members, R, **kw)()
    return r, hip.lib().bfhip_nupc_last_error()


def test_a_failing_member_changes_nothing_for_any_member(hip):
    plan = PLANS["SMALL"]
    good = GROUPS[4]
    three = good[:3]
    nu = _convolver(hip, 4, plan, fmt="S24_4LE")
    twin = _convolver(hip, 4, plan, group=0, fmt="S24_4LE")
    x = _input(plan, nu)
    flat = eq_ref.flat()
    causes = {
        "a live set": (three + [(3, 0, 0)], {}, ESTATE, b"member 3"),
        "a duplicate pair": (three + [(1, 1, 0)], {}, EINVAL, b"member 3"),
        "a filter out of range": (three + [(4, 1, 0)], {}, EINVAL, b"member 3"),
        "a set out of range": ([(0, 3, 1)] + good[1:], {}, EINVAL, b"member 0"),
        "onto_base without a base reservation": (three + [(3, 1, 1)], {}, ESTATE, b"member 3"),
        "eq_taps above the limit": (good, dict(R=512), EINVAL, b"max_taps"),
        "a zero magnitude in minimum mode": (good, dict(curve=(flat[0], [1.0, 0.0], flat[2]), mode=MINIMUM), EINVAL, b"magnitude"),
        "no members": (good, dict(n_members=0), EINVAL, b"members"),
        "more members than reserved": (good + [(0, 2, 1)], {}, EINVAL, b"members"),
    }

    def fail_all(nu):
        L = hip.lib()
        for what, (members, kw, code, text) in causes.items():
            r, msg = _call(hip, nu, members, kw.pop("R", plan["R"]), **kw)
            assert r == code and text in msg, (what, r, msg)
            assert not nu.update_busy(), what
        nu.set_coeff(3, 2)                                      # queued until the next block call
        r, msg = _call(hip, nu, three + [(3, 2, 0)], plan["R"])
        assert r == ESTATE and b"member 3" in msg and not nu.update_busy(), msg
        nu.set_coeff(3, 0)                                      # a group that changes no set commits no switch
        f, m, p = (hip._darr(list(v)) for v in CURVE)
        assert L.bfhip_nupc_render_eq_group_async(nu.h, 2, None, None, None, 256, 130, f, m, p, LINEAR) == EINVAL

    runs = [_run(nu, plan, x, {plan["b_render"]: fail_all, plan["b_switch"]: _switch(good)}),
            _run(twin, plan, x, {plan["b_switch"]: _switch(good)})]
    assert nu.switch_frame() > 0
    _same_bytes(*runs)                                          # the sets play their old contents


def test_without_the_reservation(hip):
    nu = _convolver(hip, 4, PLANS["S48 R32"], group=0)
    r, msg = _call(hip, nu, GROUPS[2], 32)
    assert r == ESTATE and b"reserve_eq_group" in msg and not nu.update_busy()
    L = hip.lib()
    assert L.bfhip_nupc_reserve_eq_group(nu.h, 4) == ESTATE      # after finalize
    raw = hip.Nupc([8, 16], [2, 2], 4, 1, 1)
    assert L.bfhip_nupc_reserve_eq_group(raw.h, 4) == ESTATE     # before reserve_eq
    raw.reserve_update()
    raw.reserve_eq(32)
    for size in (-1, 0, 1, 17, 1000):
        assert L.bfhip_nupc_reserve_eq_group(raw.h, size) == EINVAL, size
    for size in (2, 16):
        assert L.bfhip_nupc_reserve_eq_group(raw.h, size) == 0, size
    raw.close()


# ---------------------------------------------------------------- 3 (a rewrite in flight), 4: calls while a group is in flight

def _in_flight(nu, start, call, undo=lambda: None):
    """`call` directly behind `start`'s return; busy is looked at behind the call: still 1 means that the call
    was made in flight, and only such a call's answer counts.  An answer of 0 never counts: a call that starts
    a rewrite of its own is busy behind it for that reason, so it is put back and made again; a call that
    keeps answering 0 in flight fails here, after ten attempts"""
    for attempt in range(10):
        assert not nu.update_busy()
        start()
        answer = call()
        seen = nu.update_busy() and answer != 0
        assert nu.update_wait() == 0
        if seen:
            return answer
        undo()
    raise AssertionError("no attempt was both in flight and refused: answer %d" % answer)


def test_group_call_while_a_rewrite_is_in_flight(hip):
    nu, twin = _convolver(hip, 4, BIG), _convolver(hip, 4, BIG, group=0)     # 1 048 576 taps
    R, good = BIG["R"], GROUPS[4]
    single = lambda v: v.render_eq_base_async(0, 2, R, *CURVE, mode="minimum")
    r = _in_flight(nu, lambda: single(nu), _prepared(hip, nu, good, R))
    assert r == ESTATE and b"in flight" in hip.lib().bfhip_nupc_last_error()
    single(twin)
    assert twin.update_wait() == 0
    x = (np.random.default_rng(6).standard_normal((2 * nu.L0, 2)) * 0.02).astype(np.float32)
    outs = []
    for v in (nu, twin):
        _switch(good)(v)                                        # sets 1: nothing was written into them
        outs.append([v.block(x[b * v.L0:(b + 1) * v.L0]) for b in range(2)])
    for (s0, r0), (s1, r1) in zip(*outs):
        assert s0 == s1 and np.array_equal(r0, r1)


def test_calls_while_a_group_is_in_flight(hip):
    L = hip.lib()
    nu = _convolver(hip, 4, BIG)                                 # 1 048 576 taps
    h, T, R = nu.h, nu.taps, BIG["R"]
    good = GROUPS[4]
    out = np.zeros(T, np.float32)
    po = out.ctypes.data_as(C.c_void_p)
    other = _noise(41, T, np.float32)
    pt = other.ctypes.data_as(C.c_void_p)
    freq, mag, phase = (hip._darr(list(v)) for v in CURVE)
    calls = {"render_eq_group_async": _prepared(hip, nu, [(0, 2, 1), (1, 2, 0)], R),
             "render_eq_base_async": lambda: L.bfhip_nupc_render_eq_base_async(h, 0, 2, R, 130, freq, mag, phase, MINIMUM),
             "render_eq_mode_async": lambda: L.bfhip_nupc_render_eq_mode_async(h, 1, 2, R, 130, freq, mag, phase, LINEAR),
             "update_coeff_async": lambda: L.bfhip_nupc_update_coeff_async(h, 0, 2, pt, T),
             "update_coeff": lambda: L.bfhip_nupc_update_coeff(h, 0, 2, pt, T),
             "set_eq_base": lambda: L.bfhip_nupc_set_eq_base(h, 0, pt, T),
             "render_eq_mode": lambda: L.bfhip_nupc_render_eq_mode(h, R, 130, freq, mag, phase, LINEAR, po),
             "render_eq_base": lambda: L.bfhip_nupc_render_eq_base(h, 0, R, 130, freq, mag, phase, MINIMUM, po),
             "update_result": lambda: L.bfhip_nupc_update_result(h),
             "update_result_member": lambda: L.bfhip_nupc_update_result_member(h, 3),
             "set_coeff onto member 0": lambda: L.bfhip_nupc_set_coeff(h, 0, 1),
             "set_coeff onto member 3": lambda: L.bfhip_nupc_set_coeff(h, 3, 1)}
    base0 = nu.render_eq_base(0, R, *CURVE)

    def undo():
        out[:] = 0
        nu.set_eq_base(0, _noise(400, T, np.float32))
        for f in range(4):
            nu.set_coeff(f, 0)                                  # a group that changes no set commits no switch

    for what, call in calls.items():
        answer = _in_flight(nu, lambda: _group(good, R, "minimum", wait=False)(nu), call, undo)
        assert answer == ESTATE, what
        assert nu.update_result() == 0 and not np.any(out), what
        for i in range(4):
            assert nu.update_result_member(i) == 0
    assert L.bfhip_nupc_update_result_member(h, 4) == EINVAL and L.bfhip_nupc_update_result_member(h, -1) == EINVAL
    assert np.array_equal(nu.render_eq_base(0, R, *CURVE), base0)  # the base is as it was
    # and afterwards they work
    assert calls["render_eq_mode"]() == 0 and np.any(out)
    assert calls["render_eq_group_async"]() == 0 and nu.update_wait() == 0
    assert calls["update_coeff_async"]() == 0 and nu.update_wait() == 0 and nu.update_result_member(0) == 0
    assert L.bfhip_nupc_update_result_member(h, 1) == EINVAL      # a single rewrite is a group of one
    assert calls["set_coeff onto member 0"]() == 0 and calls["set_coeff onto member 3"]() == 0


# ---------------------------------------------------------------- 5: per-member result

def test_a_non_finite_member_is_reported_and_locked_alone(hip):
    plan = PLANS["SMALL"]
    T, R = 352, plan["R"]
    loud = (eq_ref.flat()[0], [1e10, 1e10], eq_ref.flat()[2])
    bases = {0: np.full(T, 1e30, np.float32), 2: _noise(402, T, np.float32)}
    # on the CPU first: these inputs overflow float32 in member 0 alone
    e = eq_ref.render(R, *loud)
    with np.errstate(over="ignore"):
        assert not np.all(np.isfinite(eq_base_ref.apply(bases[0].astype(np.float64), e, T).astype(np.float32)))
        assert np.all(np.isfinite(eq_base_ref.apply(bases[2].astype(np.float64), e, T).astype(np.float32)))
        assert np.all(np.isfinite(e.astype(np.float32))) and np.any(e)
    L = hip.lib()
    nu = _convolver(hip, 4, plan, bases=bases)
    twin = _convolver(hip, 4, plan, group=0, bases=bases)
    good = GROUPS[4]
    r, _ = _call(hip, nu, good, R, curve=loud)
    assert r == 0
    assert L.bfhip_nupc_update_wait(nu.h) == EINVAL
    assert L.bfhip_nupc_last_error() == b"NaN or Inf value among coefficients."
    assert L.bfhip_nupc_update_result(nu.h) == EINVAL
    assert [L.bfhip_nupc_update_result_member(nu.h, i) for i in range(4)] == [EINVAL, 0, 0, 0]
    assert L.bfhip_nupc_set_coeff(nu.h, 0, 1) == ESTATE
    for f in (1, 2, 3):
        nu.set_coeff(f, 1)
    # a later good rewrite unlocks the set
    h = _noise(77, T, np.float32)
    nu.update_coeff_async(0, 1, h)
    assert nu.update_wait() == 0
    nu.set_coeff(0, 1)
    # the twin: the same three renders with the single calls, the same upload
    for f, c, onto in good[1:]:
        if onto:
            twin.render_eq_base_async(f, c, R, *loud)
        else:
            twin.render_eq_async(f, c, R, *loud)
        assert twin.update_wait() == 0
    twin.update_coeff_async(0, 1, h)
    assert twin.update_wait() == 0
    _switch(good)(twin)
    x = _input(plan, nu) * 1e-9
    _same_bytes(_run(nu, plan, x, {}), _run(twin, plan, x, {}))


# ---------------------------------------------------------------- 6: purity

@pytest.mark.parametrize("rs,plan_name,mode", [(4, "SMALL", "linear"), (8, "MID", "minimum"), (4, "LONG", "minimum")])
def test_the_same_group_call_twice_gives_the_same_bytes(hip, rs, plan_name, mode):
    plan, members = PLANS[plan_name], GROUPS[4]
    runs = []
    for times in (2, 1):
        nu = _convolver(hip, rs, plan)
        runs.append(_run(nu, plan, _input(plan, nu), {plan["b_render"]: _group(members, plan["R"], mode, times=times),
                                                     plan["b_switch"]: _switch(members)}))
        assert nu.switch_frame() > 0
    _same_bytes(*runs)
