"""GPU: the linked look-ahead peak limiter on the non-uniform convolver's outputs (include/bfhip_nupc.h)
against the float64 model of tests/nupc_limiter_ref.py (held to its properties in
tests/test_nupc_limiter_model.py).

Unless a case says otherwise: a 2-in crossbar with flat-noise taps over the whole schedule
(test_gpu_nupc_chain._taps), input noise at amplitude 0.1 with bursts of x12 for 40 frames at fixed places
(one in the first frames, one across a period boundary), 48 periods through bfhip_nupc_block.  Flat-noise
taps spread a 40-frame burst over the whole response, so the level at the outputs is set by the filters'
out_scale (2: the peaks pass a threshold of 0.5 all through the run; 8 where the test needs several
times full scale).

The model's input is the device's own unlimited output: a twin convolver without a limiter, float
output format, whose bytes are x.  So only the limiter's error is measured.  Bars per sample, with x the
delayed twin sample: float32 2 * 2^-23 |x| (the envelope is float64 on both sides and rounded to the real type
once: a one-ulp flip is possible); float64 (R + D + 4) 2^-52 |x| with R = max(release_frames, 1) (the device
scans the release recursion, the model walks it: one rounding per step, which the decay bounds at about R
ulp in e, and D + 1 in the box sum); and the project's relative RMS 1e-5 / 1e-12 per channel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_limiter_ref as lr
import nupc_ref as nr
from nupc_chain_ref import IN, OUT, STAGGERED
from test_gpu_nupc_chain import _blocks, _check, _taps

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
EPS = {4: 2.0 ** -23, 8: 2.0 ** -52}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])
PERIODS = 48
ESTATE, EINVAL = -5, -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _input(rs, L0, periods, n_in=2, amp=0.1, bursts=True, burst_ch=None):
    """float raw frames in the convolver's precision; bursts of x12 for 40 frames: from frame 0 (inside
    the first D frames for every D), across the boundary of periods 4 / 5, and two more"""
    rng = np.random.default_rng(L0 + rs)
    x = rng.standard_normal((periods * L0, n_in)) * amp
    if bursts:
        cols = slice(None) if burst_ch is None else burst_ch
        for at in (0, 5 * L0 - 20, (periods // 3) * L0 + 5, (2 * periods // 3) * L0 + L0 // 2):
            x[at:at + 40, cols] *= 12.0
    return np.ascontiguousarray(x.astype(np.float32 if rs == 4 else np.float64))


def _make(hip, rs, sched, n_out, outfmt=None, wiring=None, gain=2.0, lim=None, groups=(), n_in=2, setup=None):
    """lim: (D, release) or None (the twin); groups: [(channels, threshold)]; wiring: [(in, out, out_scale)],
    default the full crossbar at out_scale `gain`"""
    dt = np.float32 if rs == 4 else np.float64
    nu = hip.Nupc(sched[0], sched[1], rs, n_in, n_out)
    nu.set_interleaved(IN, FF[rs])
    nu.set_interleaved(OUT, outfmt or FF[rs])
    rng = np.random.default_rng(7)
    for i, o, g in (wiring or [(i, o, gain) for o in range(n_out) for i in range(n_in)]):
        nu.add_filter(i, o, _taps(rng, nu.taps, dt, 1)[0].astype(dt), out_scale=g)
    if setup:
        setup(nu)
    if lim:
        nu.enable_limiter(*lim)
        for k, (chs, thr) in enumerate(groups):
            assert nu.add_limiter_group(chs, thr) == k
    nu.finalize()
    return nu


def _run(nu, x, L0, periods, before=None):
    out, sts = _blocks(nu, x, L0, periods, before)
    return out, sts


def _reals(raw, rs, n_out):
    return np.frombuffer(raw.tobytes(), np.float32 if rs == 4 else np.float64).reshape(-1, n_out).astype(np.float64)


def _bars(tag, y, want, xd, rs, D, release, chs):
    """the per-sample bar and the relative RMS bar of the module docstring on the channels chs"""
    k = 2.0 if rs == 4 else max(release, 1) + D + 4
    for c in chs:
        err = np.abs(y[:, c] - want[:, c])
        bar = k * EPS[rs] * np.abs(xd[:, c])
        worst = (err / np.maximum(bar, 1e-300)).max()
        rms = cases.rel_rms(y[:, c], want[:, c])
        print("%s rs %d ch %d: worst error / bar %.3g, rel rms %.3g" % (tag, rs, c, worst, rms))
        assert np.all(err <= bar), (c, int((err - bar).argmax()), worst)
        assert rms <= TOL[rs], (c, rms)


def _model_case(hip, tag, rs, sched, D, release, periods=PERIODS, thr=0.5):
    """one group over both outputs of a 2 x 2 crossbar against the model -> (raw bytes, reals, envelope)"""
    L0 = sched[0][0]
    dt = np.float32 if rs == 4 else np.float64
    x = _input(rs, L0, periods)
    twin = _make(hip, rs, sched, 2)
    a = _make(hip, rs, sched, 2, lim=(D, release), groups=[((0, 1), thr)])
    assert a.limiter_delay() == D and twin.limiter_delay() == 0 and a.L0 == L0
    xt, st_t = _run(twin, x, L0, periods)
    ya, st_a = _run(a, x, L0, periods)
    assert not any(st_t) and not any(st_a)
    xr = _reals(xt, rs, 2)
    want, (s,) = lr.limit(xr, [((0, 1), thr)], [1.0, 1.0], D, release, L0, dt)
    assert s.min() < 0.7 and (s == 1.0).sum() < len(s)          # it did limit
    y = _reals(ya, rs, 2)
    _bars(tag, y, want, lr.delayed(xr, D), rs, D, release, (0, 1))
    ceil = thr * (1 + (D + 4) * EPS[rs])
    assert np.abs(y).max() <= ceil and np.abs(xr).max() > thr
    twin.close()
    return a, ya, y, s


# ---------------------------------------------------------------- A. model match

@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("D,release", [(1, 0), (16, 50), (64, 500), (96, 500)])
def test_model_match(hip, rs, D, release):
    """D = 1, D < L0, D = L0 and D > L0 (the history spans periods)"""
    _model_case(hip, "A", rs, SMALL, D, release)[0].close()


# ---------------------------------------------------------------- B. period shapes

@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("sched,periods", [(([16, 32, 64], [2, 2, 4]), PERIODS),      # a period shorter than a wave
                                           (([512, 1024], [2, 2]), PERIODS),          # more than one frame per thread
                                           (([4096], [2]), 8)])                       # more than one tile
def test_period_shapes(hip, rs, sched, periods):
    _model_case(hip, "B", rs, sched, 96, 50, periods)[0].close()


@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("sched,periods", [(([4096], [2]), 8), (([16, 32, 64], [2, 2, 4]), 160)])
def test_longest_lookahead(hip, rs, sched, periods):
    """D = 1024, the contract's limit: four history values per thread, ten doubling passes, 48 KiB of LDS
    with a 1024-frame tile; and under a 16-frame period, where the history spans 64 periods"""
    _model_case(hip, "B1024", rs, sched, 1024, 50, periods)[0].close()


# ---------------------------------------------------------------- C. linking

@pytest.mark.parametrize("rs", [4, 8])
def test_linking(hip, rs):
    """groups {0, 1} (0.5) and {3} (0.25), channel 2 in none; the bursts are on input 0, which feeds
    output 0 only: output 1 is attenuated by the envelope output 0 drives"""
    D, release, L0 = 16, 50, SMALL[0][0]
    dt = np.float32 if rs == 4 else np.float64
    wiring = [(0, 0, 6.0), (1, 1, 2.0), (1, 2, 2.0), (1, 3, 2.0)]
    groups = [((0, 1), 0.5), ((3,), 0.25)]
    x = _input(rs, L0, PERIODS, burst_ch=0)
    twin = _make(hip, rs, SMALL, 4, wiring=wiring)
    a = _make(hip, rs, SMALL, 4, wiring=wiring, lim=(D, release), groups=groups)
    xt, _ = _run(twin, x, L0, PERIODS)
    ya, _ = _run(a, x, L0, PERIODS)
    xr, y = _reals(xt, rs, 4), _reals(ya, rs, 4)
    want, (s01, s3) = lr.limit(xr, groups, [1.0] * 4, D, release, L0, dt)
    assert s01.min() < 0.5 and s3.min() < 0.9 and not np.array_equal(s01, s3)
    _bars("C", y, want, lr.delayed(xr, D), rs, D, release, (0, 1, 3))
    # channel 1 alone would not have been limited that far: the shared envelope is what pulls it down
    alone = lr.envelope(lr.peaks(xr, (1,), np.array([0.5])), D, release)
    assert alone.min() > s01.min() + 0.1
    fb = 4 * rs
    got2 = ya.reshape(-1, fb)[:, 2 * rs:3 * rs]
    twin2 = xt.reshape(-1, fb)[:, 2 * rs:3 * rs]
    assert np.array_equal(got2[D:], twin2[:-D]) and not got2[:D].any() and twin2.any()
    a.close()
    twin.close()


def test_full_group(hip):
    """8 channels in one group of a 9-output convolver, the ninth in none"""
    rs, D, release, L0 = 8, 16, 50, SMALL[0][0]
    periods = 24
    groups = [(tuple(range(1, 9)), 0.5)]
    x = _input(rs, L0, periods)
    twin = _make(hip, rs, SMALL, 9)
    a = _make(hip, rs, SMALL, 9, lim=(D, release), groups=groups)
    xt, _ = _run(twin, x, L0, periods)
    ya, _ = _run(a, x, L0, periods)
    xr, y = _reals(xt, rs, 9), _reals(ya, rs, 9)
    want, (s,) = lr.limit(xr, groups, [1.0] * 9, D, release, L0)
    assert s.min() < 0.6
    _bars("C9", y, want, lr.delayed(xr, D), rs, D, release, range(1, 9))
    assert np.array_equal(y[D:, 0], xr[:-D, 0]) and not y[:D, 0].any()
    a.close()
    twin.close()


# ---------------------------------------------------------------- D. idle exactness

@pytest.mark.parametrize("rs,outfmt", [(4, None), (8, None), (8, "S24_LE")])
@pytest.mark.parametrize("kind", ["inf", "below", "nogroup"])
def test_idle_exactness(hip, rs, outfmt, kind):
    """a limiter that never limits is a pure delay of D frames: the twin's bytes, D frames later"""
    D, L0 = 96, SMALL[0][0]
    if kind == "below":
        x = _input(rs, L0, PERIODS, amp=0.02, bursts=False)
        groups = [((0, 1), 0.999)]
    else:
        x = _input(rs, L0, PERIODS)
        groups = [((0, 1), float("inf"))] if kind == "inf" else []
    twin = _make(hip, rs, SMALL, 2, outfmt=outfmt)
    a = _make(hip, rs, SMALL, 2, outfmt=outfmt, lim=(D, 500), groups=groups)
    xt, st_t = _run(twin, x, L0, PERIODS)
    ya, st_a = _run(a, x, L0, PERIODS)
    fb = len(xt) // (PERIODS * L0)
    xt, ya = xt.reshape(-1, fb), ya.reshape(-1, fb)
    assert xt.any() and np.array_equal(ya[D:], xt[:-D])
    if outfmt is None:
        assert not ya[:D].any()
    else:                                               # zeros through the quantiser
        assert np.array_equal(nr.ints(ya[:D].ravel(), bo.interleaved_formats(outfmt, 2), D), np.zeros((D, 2)))
    if groups:
        assert a.limiter_reduction(0) == 1.0
    a.close()
    twin.close()


# ---------------------------------------------------------------- E. protection

def test_protection(hip):
    """S16_LE outputs at 8x the level: the twin clips, the limited run does not"""
    rs, D, release, L0, thr = 4, 64, 500, SMALL[0][0], 0.9
    x = _input(rs, L0, PERIODS)
    twin = _make(hip, rs, SMALL, 2, outfmt="S16_LE", gain=8.0)
    a = _make(hip, rs, SMALL, 2, outfmt="S16_LE", gain=8.0, lim=(D, release), groups=[((0, 1), thr)])
    xt, _ = _run(twin, x, L0, PERIODS)
    ya, _ = _run(a, x, L0, PERIODS)
    fm = bo.interleaved_formats("S16_LE", 2)
    for c in range(2):
        print("E ch %d: twin overflows %d, limited %d" % (c, twin.overflow(c).n_overflows, a.overflow(c).n_overflows))
        assert twin.overflow(c).n_overflows > 0
        assert twin.overflow(c).largest > 3 * 32767                      # several times full scale
        assert a.overflow(c).n_overflows == 0
    v = nr.ints(ya, fm, PERIODS * L0)
    print("E: largest integer %d" % np.abs(v).max())
    assert np.abs(v).max() <= int(np.floor(thr * 32768)) + 1
    assert np.abs(v).max() >= int(np.floor(thr * 32768)) - 1             # brick wall: it goes up to the ceiling
    a.close()
    twin.close()


# ---------------------------------------------------------------- F. run-time thresholds

@pytest.mark.parametrize("rs", [4, 8])
def test_runtime_thresholds(hip, rs):
    D, release, L0 = 64, 500, SMALL[0][0]
    dt = np.float32 if rs == 4 else np.float64
    plan = {12: 0.5, 24: 0.25, 36: float("inf")}
    thr, cur = [], float("inf")
    for p in range(PERIODS):
        cur = plan.get(p, cur)
        thr.append(cur)
    x = _input(rs, L0, PERIODS)
    twin = _make(hip, rs, SMALL, 2)
    a = _make(hip, rs, SMALL, 2, lim=(D, release), groups=[((0, 1), float("inf"))])

    def before(p):
        if p in plan:
            a.set_limiter_threshold(0, plan[p])
        assert a.limiter_threshold(0) == thr[p]

    xt, _ = _run(twin, x, L0, PERIODS)
    ya, _ = _run(a, x, L0, PERIODS, before)
    xr, y = _reals(xt, rs, 2), _reals(ya, rs, 2)
    want, (s,) = lr.limit(xr, [((0, 1), thr)], [1.0, 1.0], D, release, L0, dt)
    assert np.all(s[:12 * L0] == 1.0) and s[12 * L0:24 * L0].min() < 0.8 and s[24 * L0:36 * L0].min() < s[12 * L0:24 * L0].min()
    assert s[-L0:].min() > s[24 * L0:36 * L0].min()                     # released from: the release runs
    _bars("F", y, want, lr.delayed(xr, D), rs, D, release, (0, 1))
    a.close()
    twin.close()


# ---------------------------------------------------------------- G. whole chain

def test_whole_chain(hip):
    """in one run: the limiter behind the sub-delay FIR of output 1, HP-TPDF dither on output 0 (S16), an
    output-gain ramp from 1 to 6 that drives the group into limiting, a staggered cross-faded switch, an
    integer output delay and a mute.  The bars of test_gpu_nupc_chain._check."""
    rs, sched, D, release = 8, SMALL, 64, 500
    L0 = sched[0][0]
    dt = np.float64
    ch = lr.LimitedChain(sched, rs, 2, 2, FF[rs], "S16_LE", half=15, dither=(0,))
    rng = np.random.default_rng(11)
    for o in range(2):
        for i in range(2):
            ch.add_filter(i, o, _taps(rng, ch.taps, dt, 2))
    ch.subdelay(OUT, 1, 37)
    ch.line(OUT, 1, 5, 2 * L0)
    ch.limiter(D, release)
    ch.group((0, 1), 0.5)
    nu = hip.Nupc(sched[0], sched[1], rs, 2, 2)
    nu.set_interleaved(IN, FF[rs])
    nu.set_interleaved(OUT, "S16_LE")
    nu.enable_dither([0], ch.rate)
    nu.enable_subdelay(15)
    nu.set_subdelay(OUT, 1, 37)
    nu.set_maxdelay(OUT, 1, 2 * L0)
    nu.set_delay(OUT, 1, 5)
    for f, (i, o, si, so) in enumerate(ch.filters):
        nu.add_filter(i, o, ch.h[f][0].astype(dt))
        assert nu.add_coeff(f, ch.h[f][1].astype(dt)) == 1
    nu.enable_limiter(D, release)
    assert nu.add_limiter_group([0, 1], 0.5) == 0
    nu.finalize()
    nu.set_switch_mode(STAGGERED)
    pc = ch.taps // L0 + 3
    periods = pc + (700 + 512) // L0 + 2 + (ch.taps + 700 + 512) // L0 + 2
    x = np.ascontiguousarray((rng.standard_normal((periods * L0, 2)) * 0.1).astype(dt)).view(np.uint8).reshape(periods * L0, -1)

    def before(p):
        if p == 4:
            nu.set_gain_ramp(20 * L0 + 7); nu.set_output_gain(0, 6.0); ch.set_gain(p, 0, 6.0, 20 * L0 + 7)
            nu.set_output_gain(1, 6.0); ch.set_gain(p, 1, 6.0, 20 * L0 + 7)
        if p == pc:
            nu.set_crossfade(700)
            for f in range(4):
                nu.set_coeff(f, 1)
            ch.commit(p, STAGGERED, 700, {f: (1, None) for f in range(4)})
        if p == pc + 3:
            nu.set_delay(OUT, 1, L0 + 9); ch.set_delay(p, OUT, 1, L0 + 9)
            nu.set_mute(OUT, 0, 1); ch.set_mute(p, OUT, 0, 1)
        if p == pc + 6:
            nu.set_mute(OUT, 0, 0); ch.set_mute(p, OUT, 0, 0)

    got, sts = _blocks(nu, x, L0, periods, before)
    res = ch.render(x, periods)
    assert ch.env[0].min() < 0.5 and np.all(ch.env[0][:4 * L0] == 1.0)
    _check("G", got, res, ch, periods, None, sts)
    for c in range(2):
        assert nu.overflow(c).n_overflows == res.overflow[c].n_overflows, c
    nu.close()


# ---------------------------------------------------------------- H. meter, K. purity

def test_meter_and_purity(hip):
    rs, D, release, L0 = 8, 16, 50, SMALL[0][0]
    a, raw1, y, s = _model_case(hip, "H", rs, SMALL, D, release)
    got = a.limiter_reduction(0)
    print("H: reduction %.17g, model %.17g" % (got, s.min()))
    assert abs(got - s.min()) <= (max(release, 1) + D + 4) * EPS[8]
    assert a.limiter_reduction(0) == 1.0                               # no block in between
    # the meter starts afresh: behind the filters' tail (62 periods) and the release (1 - a d rounds to 1.0
    # once d < 2^-54: 1850 frames at release 50) a period reads 1.0 again
    quiet = np.zeros((L0, 2))
    for _ in range(110):
        a.block(quiet)
    a.limiter_reduction(0)
    for _ in range(4):
        a.block(quiet)
    assert a.limiter_reduction(0) == 1.0
    a.close()
    # K: a second run gives the same bytes
    b, raw2, _, _ = _model_case(hip, "K", rs, SMALL, D, release)
    assert np.array_equal(raw1, raw2)
    b.close()


def test_purity_float32(hip):
    a, raw1, _, _ = _model_case(hip, "K", 4, SMALL, 16, 50)
    a.close()
    b, raw2, _, _ = _model_case(hip, "K", 4, SMALL, 16, 50)
    b.close()
    assert np.array_equal(raw1, raw2)


# ---------------------------------------------------------------- I. errors

def _code(nu, call):
    import brutefir_amd as bf
    with pytest.raises(bf.BfhipError) as e:
        call()
    return int(str(e.value).split("error ")[1].split(":")[0])


def test_errors(hip):
    L = hip.lib()
    nu = hip.Nupc([64], [2], 4, 2, 9)
    for o in range(9):
        nu.add_filter(0, o, np.ones(8, np.float32))
    assert _code(nu, lambda: nu.add_limiter_group([0], 0.5)) == ESTATE          # a group before enable
    for D, rel in [(0, 50.0), (1025, 50.0), (-1, 50.0), (16, 0.5), (16, -1.0), (16, float("nan")), (16, float("inf")), (16, 1.1e7)]:
        assert _code(nu, lambda: nu.enable_limiter(D, rel)) == EINVAL, (D, rel)
    assert nu.limiter_delay() == 0
    nu.enable_limiter(16, 50.0)
    assert _code(nu, lambda: nu.enable_limiter(16, 50.0)) == ESTATE             # twice
    assert nu.limiter_delay() == 16 and L.bfhip_nupc_latency(nu.h) == 64
    assert nu.add_limiter_group([0, 1], 0.5) == 0
    for chs in ([1, 2], [2, 2], [9], [-1], list(range(2, 9)) + [0, 1], []):     # in two groups, twice, range, 9, none
        assert _code(nu, lambda: nu.add_limiter_group(chs, 0.5)) == EINVAL, chs
    assert _code(nu, lambda: nu.add_limiter_group(list(range(9)), 0.5)) == EINVAL
    for thr in (0.0, -0.5, float("nan"), float("-inf")):
        assert _code(nu, lambda: nu.add_limiter_group([2], thr)) == EINVAL, thr
        assert _code(nu, lambda: nu.set_limiter_threshold(0, thr)) == EINVAL, thr
    assert _code(nu, lambda: nu.add_limiter_group([1, 3], 0.5)) == EINVAL
    assert "channel 1" in L.bfhip_nupc_last_error().decode()
    assert nu.add_limiter_group([2], float("inf")) == 1                         # nothing changed after the errors
    assert nu.limiter_threshold(0) == 0.5 and nu.limiter_threshold(1) == float("inf")
    assert _code(nu, lambda: nu.set_limiter_threshold(2, 0.5)) == EINVAL
    assert np.isnan(L.bfhip_nupc_get_limiter_threshold(nu.h, 2)) and np.isnan(L.bfhip_nupc_get_limiter_threshold(nu.h, -1))
    v = C.c_double(-3.0)
    assert L.bfhip_nupc_get_limiter_reduction(nu.h, 2, C.byref(v)) == EINVAL and v.value == -3.0
    assert L.bfhip_nupc_get_limiter_reduction(nu.h, 0, None) == EINVAL
    assert nu.limiter_reduction(0) == 1.0                                       # nothing emitted yet
    nu.finalize()
    assert _code(nu, lambda: nu.enable_limiter(16, 50.0)) == ESTATE             # after finalize
    assert _code(nu, lambda: nu.add_limiter_group([4], 0.5)) == ESTATE
    nu.set_limiter_threshold(1, 0.75)
    assert nu.limiter_threshold(1) == 0.75 and nu.limiter_delay() == 16
    st, y = nu.block(np.full((64, 2), 0.25, np.float32))
    assert st == 0 and y.any()
    nu.close()
    plain = hip.Nupc([64], [2], 4, 1, 1)
    plain.add_filter(0, 0, np.ones(8, np.float32))
    plain.finalize()
    assert _code(plain, lambda: plain.enable_limiter(16, 50.0)) == ESTATE
    assert _code(plain, lambda: plain.set_limiter_threshold(0, 0.5)) == EINVAL
    assert plain.limiter_delay() == 0
    plain.close()


# ---------------------------------------------------------------- J. other paths

def test_block_dev_gives_the_bytes_of_block(hip):
    import torch
    rs, D, release, L0, periods = 4, 96, 50, SMALL[0][0], 16
    x = _input(rs, L0, periods)
    groups = [((0, 1), 0.5)]
    a = _make(hip, rs, SMALL, 2, lim=(D, release), groups=groups)
    b = _make(hip, rs, SMALL, 2, lim=(D, release), groups=groups)
    ya, _ = _run(a, x, L0, periods)
    xd = torch.from_numpy(x).cuda()
    yd = torch.zeros((periods * L0, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for p in range(periods):
        b._chk(hip.lib().bfhip_nupc_block_dev(b.h, C.c_void_p(xd[p * L0:].data_ptr()), C.c_void_p(yd[p * L0:].data_ptr())))
    assert b.sync() == 0
    yb = yd.cpu().numpy().view(np.uint8).ravel()
    assert ya.any() and np.array_equal(ya, yb)
    a.close()
    b.close()


def test_planar_output_buffer(hip):
    """a declared output buffer of two planes: sample for sample the interleaved run's values"""
    rs, D, release, L0, periods = 4, 16, 50, SMALL[0][0], 16
    x = _input(rs, L0, periods)
    groups = [((0, 1), 0.5)]
    a = _make(hip, rs, SMALL, 2, lim=(D, release), groups=groups)

    def planes(nu):
        for c in range(2):
            nu.set_format(OUT, c, hip.make_format(FF[rs], 1, c * L0 * rs))
        nu.set_buffer_bytes(OUT, 2 * L0 * rs)

    b = _make(hip, rs, SMALL, 2, lim=(D, release), groups=groups, setup=planes)
    ya, _ = _run(a, x, L0, periods)
    yb, _ = _run(b, x, L0, periods)
    va = np.frombuffer(ya.tobytes(), np.float32).reshape(periods, L0, 2)
    vb = np.frombuffer(yb.tobytes(), np.float32).reshape(periods, 2, L0).transpose(0, 2, 1)
    assert va.any() and np.array_equal(va, vb)
    a.close()
    b.close()


def test_background_off_in_a_child(hip, tmp_path):
    """BFHIP_NUPC_BACKGROUND=0 (every segment on the main stream) in a fresh process: the model's bars"""
    env = dict(os.environ, BFHIP_NUPC_BACKGROUND="0")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import conftest, test_gpu_nupc_limiter as t\n"
            "conftest._init_torch()\n"
            "import brutefir_amd as bf\n"
            "t._model_case(bf, 'J', 8, t.SMALL, 96, 500)[0].close()\n"
            "t._model_case(bf, 'J', 4, t.SMALL, 96, 500)[0].close()\n"
            "print('child ok')\n" % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


# ---------------------------------------------------------------- L. allocation faults

def test_every_allocation_failure_is_an_error_code(hip):
    """create ... finalize ... one block ... destroy of a limiter convolver with the n-th allocation failing,
    n = 1, 2, ... until a life no longer reaches the armed allocation: each failure is a BfhipError, destroy
    cleans up what was half built, and a clean life works afterwards"""
    L = hip.lib()
    x = _input(4, 64, 1)
    left = [0]

    def life():
        nu = None
        try:
            nu = hip.Nupc([64, 128], [2, 2], 4, 2, 3)
            for o in range(3):
                nu.add_filter(o % 2, o, np.ones(100, np.float32) / 8)
            nu.enable_limiter(96, 50.0)
            nu.add_limiter_group([0, 2], 0.5)
            nu.finalize()
            return np.concatenate([nu.block(x)[1] for _ in range(3)])       # the look-ahead is a period and a half
        finally:
            left[0] = L.bfhip_selftest_fail_alloc(0)
            if nu is not None:
                nu.close()

    want = life()
    n, errors, absorbed = 0, 0, 0
    while True:
        n += 1
        assert n < 400
        L.bfhip_selftest_fail_alloc(n)
        try:
            got = life()
        except hip.BfhipError:
            assert left[0] == 0, "an error without the armed allocation"
            errors += 1
            continue
        if left[0] > 0:
            break                                        # a whole life makes n - left allocations
        absorbed += 1
        assert np.array_equal(got, want)
    print("L: %d allocations walked, %d errors, %d absorbed" % (n - 1, errors, absorbed))
    assert errors + absorbed == n - 1 and errors >= 19 and absorbed <= 6   # finalize alone makes 19 of its own
    assert np.array_equal(life(), want) and want.any()
