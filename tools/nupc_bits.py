"""sha256 of the output periods of a fixed list of non-uniform convolver cases, from seeded numpy inputs.

    python tools/nupc_bits.py [--out FILE] [case ...]

One JSON object {case: {"sha256": ..., "nonzero": true, "ran": true}}.  Run on the commit before csrc/nupc.hip
was taken apart (ee5807d) and committed as tests/golden/nupc_bits_parent.json, it pins what the moved host
code decides per period: which assignment a segment block runs under, which ring it is added to, whether
it fades and from which frame, when the rings flip, where a gain ramp stands, which delay job a channel
gets, which sub-delay values and formats the kernels are handed.  A decision taken one period early or
late, or an argument taken from the wrong field, changes bits below any tolerance.
tests/test_gpu_nupc_bits.py asserts the same values on the tree it runs in.

Every case is tests/nupc_stagger_ref.py's 2 x 2 crossbar (flat-noise impulse responses over the whole
schedule, the sets of a filter different in every segment), L0 = 64, 40 periods through
bfhip_nupc_block (one sync per period), float I/O of the convolver's precision unless the case says
otherwise.  SMALL has its segments behind the first in the background; ZERO has every segment on the
main stream.  Periods are hashed in order.

`ran`: what the binding exposes says the case's branch was taken (switch frames, busy flags, get_delay,
get_subdelay, update_result ...).  `differs`: the case must not hash like the named one (a gain, a
dither, a rewrite that never reached the device would).  `twin`: cases the parent run showed to hash
equal: the asynchronous rewrite and the synchronous one.  Background on and off are not twins: they
accumulate in a different order.
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nupc_stagger_ref as sr  # noqa: E402
from nupc_stagger_ref import SMALL, ZERO  # noqa: E402

L0, PERIODS = 64, 40
IN, OUT = 0, 1
ENV_KEYS = ("BFHIP_NUPC_BACKGROUND",)
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
ALL = range(4)


@contextlib.contextmanager
def env_set(**kv):
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    assert set(kv) <= set(ENV_KEYS), kv
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---------------------------------------------------------------- steps: before(nu, st), at(b, nu, st), ran(nu, st)

def _switch_all(nu, c, fade=None):
    if fade is not None:
        nu.set_crossfade(fade)
    for f in ALL:
        nu.set_coeff(f, c)


def _seg_frames(nu, st):
    return [nu.switch_frame_segment(k) for k in range(len(st["sched"][0]))]


def switch_at_5(fade, staggered=False):
    """one switch of every filter to set 1, requested before block 5: t_req = 320, where the segments'
    grids disagree"""
    def before(bf, nu, st):
        if staggered:
            nu.set_switch_mode(bf.SWITCH_STAGGERED)

    def at(b, nu, st):
        if b == 5:
            _switch_all(nu, 1, fade)
        if b == 6:
            st["frames"] = _seg_frames(nu, st)
            st["t_sw"] = nu.switch_frame()
            st["busy"] = nu.switch_busy()

    def ran(nu, st):
        want = sr.switch_frames(st["sched"], 5 * L0)
        if staggered:
            return (st["t_sw"] == 5 * L0 and st["frames"] == want and len(set(want)) > 1
                    and st["busy"] == (fade > 0) and not nu.switch_busy())
        return (st["t_sw"] == max(want) > 5 * L0 and st["frames"] == [max(want)] * len(want) and st["busy"]
                and not nu.switch_busy())
    return dict(sets=2, before=before, at=at, ran=ran)


def two_switches(first_staggered):
    """to set 1 before block 5, and back onto set 0 (aligned) in the first period the convolver is no
    longer busy"""
    def before(bf, nu, st):
        st["bf"] = bf
        if first_staggered:
            nu.set_switch_mode(bf.SWITCH_STAGGERED)

    def at(b, nu, st):
        if b == 5:
            _switch_all(nu, 1, 64)
        if b == 6:
            st["first"] = (nu.switch_frame(), _seg_frames(nu, st))
        if b > 5 and "second_at" not in st and not nu.switch_busy():
            if first_staggered:
                nu.set_switch_mode(st["bf"].SWITCH_ALIGNED)
            _switch_all(nu, 0, 64)
            st["second_at"] = b
        if "second_at" in st and b == st["second_at"] + 1:
            st["second"] = (nu.switch_frame(), _seg_frames(nu, st))

    def ran(nu, st):
        t1, f1 = st["first"]
        t2, f2 = st["second"]
        w2 = max(sr.switch_frames(st["sched"], st["second_at"] * L0))
        return (t1 >= 5 * L0 and (len(set(f1)) > 1) == first_staggered and t2 == w2 > t1 and f2 == [w2] * len(f2)
                and st["second_at"] < PERIODS - 12 and not nu.switch_busy())
    return dict(sets=2, before=before, at=at, ran=ran)


def gain_only():
    def before(bf, nu, st):
        nu.reserve_filter_gain()

    def at(b, nu, st):
        if b == 5:
            nu.set_filter_gain(0, 0.5)
            nu.set_filter_gain(3, -1.5)

    def ran(nu, st):
        return nu.switch_frame() > 5 * L0 and nu.get_filter_gain(0) == 0.5 and nu.get_filter_gain(3) == -1.5 \
            and nu.get_filter_gain(1) == 1.0 and not nu.switch_busy()
    return dict(before=before, at=at, ran=ran)


def output_gain(ramp):
    """a step or a 200-frame ramp before block 5 on both outputs; output 1 gets a second request before
    block 7, in mid-ramp"""
    def before(bf, nu, st):
        nu.set_gain_ramp(ramp)

    def at(b, nu, st):
        if b == 5:
            nu.set_output_gain(0, 0.25)
            nu.set_output_gain(1, 2.0)
        if b == 7:
            nu.set_output_gain(1, -0.5)
    return dict(before=before, at=at, ran=lambda nu, st: True)


def dither():
    def before(bf, nu, st):
        nu.enable_dither([1], 44100)
    return dict(out_fmt="S24_4LE", before=before, ran=lambda nu, st: True)


def delays():
    """maxdelay 200 on input 0 and output 1: 0 -> 30 -> 130 -> 64 -> 0 across F = 64 on both sides, the two
    sides two periods apart; input 1 muted over periods 8 .. 11, output 0 over 20 .. 22"""
    walk = {4: 30, 10: 130, 16: 64, 22: 0}

    def before(bf, nu, st):
        nu.set_maxdelay(IN, 0, 200)
        nu.set_maxdelay(OUT, 1, 200)
        st["seen"] = []

    def at(b, nu, st):
        if b in walk:
            nu.set_delay(IN, 0, walk[b])
        if b - 2 in walk:
            nu.set_delay(OUT, 1, walk[b - 2])
        if b - 1 in walk:
            st["seen"].append(nu.get_delay(IN, 0) == walk[b - 1])
        if b - 3 in walk:
            st["seen"].append(nu.get_delay(OUT, 1) == walk[b - 3])
        if b in (8, 12):
            nu.set_mute(IN, 1, b == 8)
        if b in (20, 23):
            nu.set_mute(OUT, 0, b == 20)

    def ran(nu, st):
        return len(st["seen"]) == 8 and all(st["seen"]) and nu.get_delay(IN, 1) == 0
    return dict(before=before, at=at, ran=ran)


def subdelay():
    """31-tap filters on input 0 and output 0; input 1 and output 1 have none and follow 15 frames later"""
    def before(bf, nu, st):
        nu.enable_subdelay(15)
        nu.set_subdelay(IN, 0, 37)
        nu.set_subdelay(OUT, 0, -42)
        st["undef"] = bf.UNDEFINED_SUBDELAY

    def at(b, nu, st):
        if b == 9:
            nu.set_subdelay(IN, 0, -80)
        if b == 13:
            nu.set_subdelay(OUT, 0, 99)

    def ran(nu, st):
        return [nu.get_subdelay(io, ch) for io in (IN, OUT) for ch in (0, 1)] == [-80, st["undef"], 99, st["undef"]]
    return dict(before=before, at=at, ran=ran)


def planar():
    def ran(nu, st):
        return nu.buffer_bytes(IN) == st["nbytes"] and nu.buffer_bytes(OUT) == st["nbytes"]
    return dict(planar=True, ran=ran)


def _new_taps(st, f):
    rng = np.random.default_rng(900 + f)
    return (rng.standard_normal(st["taps"]) / np.sqrt(st["taps"])).astype(st["dt"])


def rewrite(asynchronous):
    """set 1 of every filter rewritten before block 3 while idle, switched to before block 5"""
    def before(bf, nu, st):
        if asynchronous:
            nu.reserve_update()

    def at(b, nu, st):
        if b == 3:
            for f in ALL:
                if asynchronous:
                    nu.update_coeff_async(f, 1, _new_taps(st, f))
                    st.setdefault("results", []).append(nu.update_wait())
                else:
                    nu.update_coeff(f, 1, _new_taps(st, f))
        if b == 5:
            _switch_all(nu, 1, 64)

    def ran(nu, st):
        return nu.switch_frame() > 5 * L0 and not nu.switch_busy() and \
            (not asynchronous or (st["results"] == [0] * 4 and not nu.update_busy()))
    return dict(sets=2, before=before, at=at, ran=ran)


def render_eq(mode):
    """a 2048-tap curve per filter rendered on the device into set 1 before block 3, switched to before block 5"""
    freq = [0.0, 0.01, 0.05, 0.2, 0.35, 0.5]

    def before(bf, nu, st):
        nu.reserve_update()
        nu.reserve_eq(2048)
        nu.reserve_eq_minimum()

    def at(b, nu, st):
        if b == 3:
            for f in ALL:
                mag = [1.0, 0.5 + 0.25 * f, 2.0, 0.75, 1.5 - 0.25 * f, 0.125]
                phase = [0.0, 0.3, -0.2 * f, 0.4, 0.0, 0.0]
                nu.render_eq_async(f, 1, 2048, freq, mag, phase, mode=mode)
                st.setdefault("results", []).append(nu.update_wait())
        if b == 5:
            _switch_all(nu, 1, 64)

    def ran(nu, st):
        return st["results"] == [0] * 4 and nu.switch_frame() > 5 * L0 and not nu.switch_busy()
    return dict(sets=2, before=before, at=at, ran=ran)


# ---------------------------------------------------------------- cases

def case_list():
    """name -> dict(sched, rs, env, seed, sets, out_fmt, planar, before, at, ran, differs, twin)"""
    cs = {}

    def add(name, sched=SMALL, rs=4, env=None, differs=None, twin=None, **steps):
        c = dict(sched=sched, rs=rs, env=env or {}, seed=71, sets=1, out_fmt=None, planar=False, before=None, at=None,
                 ran=lambda nu, st: True, differs=differs, twin=twin)
        c.update(steps)
        cs[name] = c

    for rs in (4, 8):
        add("plain_f%d_small" % (rs * 8), SMALL, rs)
        add("plain_f%d_zero" % (rs * 8), ZERO, rs)
    add("plain_f32_small_no_background", env={"BFHIP_NUPC_BACKGROUND": 0})
    for F in (0, 2, 64, 323):
        add("aligned_fade%d" % F, differs="plain_f32_small", **switch_at_5(F))
    add("aligned_fade64_zero", ZERO, differs="plain_f32_zero", **switch_at_5(64))
    add("aligned_fade64_f64", rs=8, differs="plain_f64_small", **switch_at_5(64))
    add("aligned_twice", differs="aligned_fade64", **two_switches(False))
    for F in (0, 323):
        add("staggered_fade%d" % F, differs="aligned_fade%d" % F, **switch_at_5(F, staggered=True))
    add("staggered_fade323_zero", ZERO, differs="plain_f32_zero", **switch_at_5(323, staggered=True))
    add("staggered_then_aligned", differs="aligned_twice", **two_switches(True))
    add("gain_only_switch", differs="plain_f32_small", **gain_only())
    add("output_gain_step", differs="plain_f32_small", **output_gain(0))
    add("output_gain_ramp200", differs="output_gain_step", **output_gain(200))
    add("s24_out", out_fmt="S24_4LE")
    add("s24_out_dither", differs="s24_out", **dither())
    add("delay_mute", differs="plain_f32_small", **delays())
    add("subdelay", differs="plain_f32_small", **subdelay())
    add("subdelay_f64_zero", ZERO, 8, differs="plain_f64_zero", **subdelay())
    add("planar", **planar())
    add("update_coeff", differs="aligned_fade64", **rewrite(False))
    add("update_coeff_async", differs="aligned_fade64", twin="update_coeff", **rewrite(True))
    add("render_eq_linear", differs="aligned_fade64", **render_eq("linear"))
    add("render_eq_minimum", differs="render_eq_linear", **render_eq("minimum"))
    return cs


def run_case(c):
    """-> {"sha256", "nonzero", "ran"}"""
    import torch
    assert torch.cuda.is_available()     # torch's own HIP runtime has to start before libbfhip.so loads the system's
    import brutefir_amd as bf
    rs, sched = c["rs"], c["sched"]
    dt = np.float32 if rs == 4 else np.float64
    cb = sr.Crossbar(sched, c["sets"], c["seed"], L0 * PERIODS, dt)
    st = {"sched": sched, "taps": cb.taps, "dt": dt}
    with env_set(**c["env"]):
        nu = bf.Nupc(sched[0], sched[1], rs, 2, 2)
        try:
            if c["planar"]:
                fmts, st["nbytes"] = bf.period_layout(L0, [(FF[rs], 2, [0, 1], False)])
                for io in (IN, OUT):
                    for ch, f in enumerate(fmts):
                        nu.set_format(io, ch, f)
                    nu.set_buffer_bytes(io, st["nbytes"])
            else:
                nu.set_interleaved(IN, FF[rs])
                nu.set_interleaved(OUT, c["out_fmt"] or FF[rs])
            for f in ALL:
                nu.add_filter(f % 2, f // 2, cb.h[f][0], in_scale=cb.in_scale[f], out_scale=cb.out_scale[f])
                for j in range(1, c["sets"]):
                    assert nu.add_coeff(f, cb.h[f][j]) == j
            if c["before"]:
                c["before"](bf, nu, st)
            nu.finalize()
            got = []
            for b in range(PERIODS):
                if c["at"]:
                    c["at"](b, nu, st)
                x = cb.x[b * L0:(b + 1) * L0]
                status, raw = nu.block(np.ascontiguousarray(x.T) if c["planar"] else x)
                assert status == 0, (b, status)
                got.append(raw.tobytes())
            assert nu.sync() == 0
            ran = bool(c["ran"](nu, st))
        finally:
            nu.close()
    h = hashlib.sha256()
    for g in got:
        h.update(g)
    return {"sha256": h.hexdigest(), "nonzero": all(any(g) for g in got[-2:]), "ran": ran}


def main(argv):
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    cs = case_list()
    names = argv or list(cs)
    res = {}
    for n in names:
        res[n] = run_case(cs[n])
        print(n, res[n], file=sys.stderr, flush=True)
    for n in names:
        for key in ("twin", "differs"):
            t = cs[n][key]
            if t in res:
                print(key, n, t, "equal" if res[n]["sha256"] == res[t]["sha256"] else "not equal", file=sys.stderr, flush=True)
    by_hash = {}
    for n in names:
        by_hash.setdefault(res[n]["sha256"], []).append(n)
    for group in by_hash.values():
        if len(group) > 1:
            print("hash equal:", group, file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1, sort_keys=True) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    bad = [n for n in names if not (res[n]["nonzero"] and res[n]["ran"])]
    assert not bad, bad


if __name__ == "__main__":
    main(sys.argv[1:])
