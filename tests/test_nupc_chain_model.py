"""CPU: the float64 chain model of the non-uniform convolver (tests/nupc_chain_ref.py) that
tests/test_gpu_nupc_chain.py compares the device against is itself checked -- with every control
off it is nupc_ref.convolve + encode byte for byte, its delay line at L0 = 64 is the one the delay
tests have always used, a staggered commit with equal switch frames is the aligned one, its gain
record is the header's formula, and the session generator keeps its promises."""
import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_chain_ref as cr
import nupc_ref as nr
import nupc_stagger_ref as sr
from nupc_chain_ref import ALIGNED, IN, OUT, STAGGERED

SMALL = sr.SMALL


def _raw(rng, fmt, frames, n_ch, amp=0.1):
    nbytes, sbytes, isfloat, _ = bo.SAMPLE_FORMATS[fmt]
    x = rng.standard_normal((frames, n_ch)) * amp
    if isfloat:
        return x.astype(np.float32 if nbytes == 4 else np.float64).view(np.uint8).reshape(frames, -1)
    full = 1 << (8 * sbytes - 1)
    v = np.clip(np.round(x * full), -full, full - 1).astype("<i8")
    return np.ascontiguousarray(v.view(np.uint8).reshape(frames, n_ch, 8)[:, :, :nbytes]).reshape(frames, -1)


def _crossbar(sched, rs, infmt, outfmt, seed, n_sets=1, **kw):
    ch = cr.Chain(sched, rs, 2, 2, infmt, outfmt, **kw)
    rng = np.random.default_rng(seed)
    for f in range(4):
        sets = [rng.standard_normal(ch.taps) / np.sqrt(ch.taps) for _ in range(n_sets)]
        ch.add_filter(f % 2, f // 2, sets, in_scale=0.5 if f % 2 else 1.0, out_scale=-1.0 if f // 2 else 1.0)
    return ch


@pytest.mark.parametrize("infmt,outfmt,dither", [("S16_LE", "S24_LE", ()), ("FLOAT64_LE", "S16_LE", (0, 1)),
                                                 ("S24_4LE", "FLOAT_LE", ())])
def test_every_control_off_is_convolve_and_encode(infmt, outfmt, dither):
    periods, L0 = 30, 64
    ch = _crossbar(SMALL, 8, infmt, outfmt, 3, dither=dither)
    x = _raw(np.random.default_rng(4), infmt, periods * L0, 2, 0.3)
    got = ch.render(x, periods)
    xr = nr.decode(x.ravel(), ch.fmts[IN], periods * L0)
    y = nr.convolve(xr, [(i, o, ch.h[f][0], si, so) for f, (i, o, si, so) in enumerate(ch.filters)], 2)
    # the per-segment sums differ from the one convolution in the last bits of float64: rounded to
    # the same integers but at ties, so the float path is compared first
    assert cases.rel_rms(got.reals, y) <= 1e-13
    raw, of, st = nr.encode(got.reals, ch.fmts[OUT], L0, dither=dither, rate=300)
    assert np.array_equal(got.raw, raw) and got.status == st
    assert [o.astuple() for o in got.overflow] == [o.astuple() for o in of]
    want, _, _ = nr.encode(y, ch.fmts[OUT], L0, dither=dither, rate=300)
    assert np.array_equal(got.raw, want)


def _old_line_run(lines, muted, req, io, raw, nbytes):
    """the delay tests' model as it stood before it took L0 as a parameter: bfo_delay_update with a
    fragment of 64 on every channel's samples, mute in dai.c's order"""
    fr = np.ascontiguousarray(raw).view(np.uint8).reshape(64, -1).copy()
    for ch, d in enumerate(lines):
        s = np.ascontiguousarray(fr[:, ch * nbytes:(ch + 1) * nbytes])
        if io == IN and muted[ch]:
            s[:] = 0
        cr._olib().bfo_delay_update(d, s.ctypes.data, int(req[ch]))
        if io == OUT and muted[ch]:
            s[:] = 0
        fr[:, ch * nbytes:(ch + 1) * nbytes] = s
    return fr.ravel()


@pytest.mark.parametrize("io,fmt", [(IN, "S16_LE"), (OUT, "S24_LE"), (IN, "FLOAT64_LE"), (OUT, "S32_LE")])
def test_parametrised_line_is_the_old_one_at_64(io, fmt):
    """the seeded changes of test_random_delay_changes_and_mute_toggles, its specs and choices"""
    L0, periods, n_ch = 64, 150, 3
    spec = [(10, 3 * L0 + 10), (20, -1), (L0, L0)] if io == IN else [(0, 5 * L0), (2 * L0 - 3, 2 * L0 - 3), (70, -1)]
    nbytes = bo.SAMPLE_FORMATS[fmt][0]
    m = cr.Model(io, fmt, spec, L0)
    old = [cr._olib().bfo_delay_new(64, d, mx, nbytes) for d, mx in spec]
    req, muted = [d for d, _ in spec], [False] * n_ch
    rng = np.random.default_rng(1)
    x = _raw(rng, fmt, periods * L0, n_ch, 0.3)
    choices = [0, 1, L0 - 1, L0, L0 + 1, 2 * L0 - 3, 2 * L0, 2 * L0 + 17, 3 * L0 + 10, 5 * L0, 5 * L0 + 1, 9 * L0]
    for p in range(periods):
        for c in range(n_ch):
            if rng.random() < 0.2:
                req[c] = m.lines[c].req = int(rng.choice(choices))
            if rng.random() < 0.08:
                muted[c] = m.lines[c].muted = not muted[c]
        xb = x[p * L0:(p + 1) * L0]
        assert np.array_equal(m.run(xb), _old_line_run(old, muted, req, io, xb, nbytes)), p
    for d in old:
        cr._olib().bfo_delay_free(d)


@pytest.mark.parametrize("L0,nbytes", [(256, 3), (512, 2), (4096, 8)])
def test_line_is_a_pure_delay_at_any_fragment(L0, nbytes):
    """steady delays below, at and above the fragment: the stream d samples late"""
    rng = np.random.default_rng(L0)
    x = rng.integers(1, 255, (8 * L0, nbytes), dtype=np.uint8)
    for d in (1, L0 - 1, L0, L0 + 1, 3 * L0 + 7):
        ln = cr.Line(IN, d, -1, nbytes, L0)
        out = []
        for p in range(8):
            fr = x[p * L0:(p + 1) * L0].copy()
            ln.run(fr, 0)
            out.append(fr)
        out = np.concatenate(out)
        assert not out[:d].any() and np.array_equal(out[d:], x[:len(x) - d]), d


@pytest.mark.parametrize("F", [0, 2, 64, 700])
def test_staggered_commit_with_equal_frames_is_the_aligned_one(F):
    periods, L0 = 60, 64
    x = _raw(np.random.default_rng(6), "FLOAT64_LE", periods * L0, 2)
    out = []
    for mode in (ALIGNED, STAGGERED):
        ch = _crossbar(SMALL, 8, "FLOAT64_LE", "FLOAT64_LE", 5, n_sets=2)
        ch.commit(7, mode, F, {f: (1, None) for f in range(4)})
        ch.commit(40, mode, 64, {0: (0, -0.5), 3: (None, 0.0)})
        t = {p * L0: [cr.aligned_frame(SMALL, p * L0)] * 4 for p in (7, 40)}
        out.append(ch.render(x, periods, frames=lambda t_req: t[t_req]).reals)
    assert cr.aligned_frame(SMALL, 7 * L0) == 7 * L0 + 448          # 896 of the 512 segment
    assert cases.rel_rms(out[1], out[0]) <= 1e-13
    # and left to the formula the staggered run differs: the head switches first
    ch = _crossbar(SMALL, 8, "FLOAT64_LE", "FLOAT64_LE", 5, n_sets=2)
    ch.commit(7, STAGGERED, F, {f: (1, None) for f in range(4)})
    ch.commit(40, STAGGERED, 64, {0: (0, -0.5), 3: (None, 0.0)})
    y = ch.render(x, periods).reals
    # (in the aligned run the first period is still all old; a 700-frame fade has moved 64 / 699 by its end)
    assert cases.rel_rms(y[7 * L0:8 * L0], out[0][7 * L0:8 * L0]) > 0.01


def test_a_rewritten_set_is_heard_with_the_taps_it_held_at_the_commit():
    periods, L0 = 50, 64
    x = _raw(np.random.default_rng(8), "FLOAT64_LE", periods * L0, 2)
    ch = _crossbar(SMALL, 8, "FLOAT64_LE", "FLOAT64_LE", 9, n_sets=2)
    fresh = np.random.default_rng(10).standard_normal(ch.taps) / np.sqrt(ch.taps)
    ch.commit(3, ALIGNED, 0, {f: (1, None) for f in range(4)})
    ch.update(2, 0, fresh)
    ch.commit(30, STAGGERED, 0, {2: (0, None)})
    y = ch.render(x, periods).reals
    xr = nr.decode(x.ravel(), ch.fmts[IN], periods * L0)
    last = [(i, o, (fresh if f == 2 else ch.h[f][1]), si, so) for f, (i, o, si, so) in enumerate(ch.filters)]
    first = [(i, o, ch.h[f][0], si, so) for f, (i, o, si, so) in enumerate(ch.filters)]
    assert cases.rel_rms(y[30 * L0 + ch.taps:], nr.convolve(xr, last, 2)[30 * L0 + ch.taps:]) <= 1e-12
    assert np.allclose(y[:3 * L0], nr.convolve(xr, first, 2)[:3 * L0], rtol=0, atol=1e-14)


def test_gain_ramp_is_the_record_of_the_schedule():
    """frame idx of a ramp of len frames: a + (g - a)(idx + 1) / len below len - 1, then g; a new
    target mid-ramp starts from the last emitted frame's gain; the same target again does not"""
    L0 = 64
    gr = cr.GainRamp(10 * L0, L0, [1.0, 2.0])
    gr.set_ramp(150)
    gr.request(0, 0.25)
    gr.commit(1)
    gr.request(0, 0.25)
    gr.commit(2)                                  # same target mid-ramp: nothing restarts
    idx = np.arange(150)
    want = np.where(idx < 149, 1.0 + (0.25 - 1.0) * ((idx + 1) / 150.0), 0.25)      # the device's order
    assert np.array_equal(gr.g[L0:L0 + 150, 0], want) and np.all(gr.g[L0 + 150:, 0] == 0.25)
    assert np.all(gr.g[:L0, 0] == 1.0) and np.all(gr.g[:, 1] == 2.0)
    gr.set_ramp(0)
    gr.request(1, 0.5)
    gr.request(1, 3.0)                            # the last call counts; its ramp length is in force
    gr.set_ramp(64)
    gr.request(0, 1.0)
    gr.commit(3)                                  # frame 192: channel 0 is at 1 - .75 * 129 / 150
    a = 1.0 + (0.25 - 1.0) * (128 / 150.0)
    assert gr.g[3 * L0 - 1, 0] == a
    assert gr.g[3 * L0, 0] == a + (1.0 - a) * (1 / 64.0) and gr.g[4 * L0 - 1, 0] == 1.0
    assert np.all(gr.g[3 * L0:, 1] == 3.0) and gr.g[3 * L0 - 1, 1] == 2.0


@pytest.mark.parametrize("seed", range(8))
def test_session_generator(seed):
    s, again = cr.session(seed), cr.session(seed)
    assert repr(s) == repr(again)
    assert s["rs"] == (4, 8)[seed % 2]
    kinds = [k for _, k, _ in s["events"]]
    for k in cr.KINDS:
        assert k in kinds, k
    assert [p for p, _, _ in s["events"]] == sorted(p for p, _, _ in s["events"])
    sched = s["sched"]
    L0, Lmax = sched[0][0], sched[0][-1]
    taps = sum(L * N for L, N in zip(*sched))
    commits = [(p, a[1]) for p, k, a in s["events"] if k == "commit"]
    assert len(commits) >= 3
    for (p0, F0), (p1, _) in zip(commits, commits[1:]):
        assert (p1 - p0) * L0 >= taps + F0 + 2 * Lmax
    assert (s["periods"] - commits[-1][0]) * L0 >= taps + commits[-1][1] + 2 * Lmax
    # an update rewrites a set that is idle -- no commit names it, and the commit before it is at
    # least taps + F + 2 L_max frames back, so no switch is in flight -- and a later commit switches onto it
    for p, k, a in s["events"]:
        if k == "update":
            before = [(q, F) for q, F in commits if q <= p]
            assert before and (p - before[-1][0]) * L0 >= taps + before[-1][1] + 2 * Lmax
            assert a[1] == 0 and all(b[2].get(a[0], (None,))[0] != 0 for q, c, b in s["events"] if c == "commit" and q <= p)
            assert any(q > p and c == "commit" and b[2].get(a[0], (None,))[0] == a[1] for q, c, b in s["events"])
    assert 2 * s["half"] + 1 <= L0
    if s["rs"] == 4:
        assert not s["dither"] and s["outfmt"] in ("S16_LE", "FLOAT_LE")
    if s["dither"]:
        assert s["outfmt"] in ("S16_LE", "S24_LE")


def test_sessions_cover_the_schedules_and_both_modes():
    ss = [cr.session(seed) for seed in range(8)]
    assert {tuple(map(tuple, s["sched"])) for s in ss} == {tuple(map(tuple, c)) for c in cr.SESSION_SCHEDS}
    modes = {(s["rs"], a[0]) for s in ss for _, k, a in s["events"] if k == "commit"}
    assert modes == {(4, ALIGNED), (4, STAGGERED), (8, ALIGNED), (8, STAGGERED)}
    assert any(s["dither"] for s in ss)
