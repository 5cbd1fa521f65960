"""GPU: the limiter's true-peak detector (bfhip_nupc_set_limiter_detector, include/bfhip_nupc.h) against the
float64 model of tests/nupc_truepeak_ref.py (held to its properties in tests/test_nupc_truepeak_model.py).

As in tests/test_gpu_nupc_limiter.py the model's input is the device's own unlimited output: a twin convolver
without a limiter and with float outputs, whose bytes are x, so only the limiter's error is measured.  Two
kinds of filters: flat-noise taps over the whole (short) schedule on a 2-in crossbar, for noise with bursts;
and one-tap filters, out o from in o % 2, which put a sine or single impulses where the test wants them.

Bars per sample, with x the twin sample D frames earlier, D_e = D - H, R = max(release_frames, 1):

    float64   ((R + D_e + 4) 2^-52 + K) |x|,   K = 2 H 2^-52 max_q ||g_q||_1 max|x| / min ceil
              The first term is the existing limiter test's (scan against walk in the release recursion, box
              sum) with the envelope's look-ahead.  K: device and model both form u_q as a 24-term float64 sum, k
              ascending, the device with fused multiply-adds; each is within gamma_24 sum |g_q[k]| |x[t - k]| <=
              24 2^-53 ||g_q||_1 max|x| of the exact sum, so they differ by at most 2 H 2^-52 ||g_q||_1 max|x| in
              u and by that over ceil in p.  r = 1 / p where p > 1, so |dr| = |dp| / p^2 <= |dp| (a p that falls
              on the other side of 1 gives r = 1 against 1 / p: within |dp| too).  Window minimum, release
              recursion (a <= 1) and box mean are monotone and move by no more than their inputs do, so |ds| <=
              max |dr| <= K, and y = x s moves by K |x|.
    float32   the float64 bar + 2 * 2^-23 |x|: s is float64 on both sides and rounded to T once; where the two
              roundings fall apart, (T) s differs by one ulp of T (up to 2^-23 of s, just above a power of two)
              and the two rounded products by up to another 2^-23 |y|
    integer outputs   the bar in counts + 1 (the quantiser's rounding)
and the project's relative RMS 1e-5 / 1e-12 per channel."""
import ctypes as C

import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_limiter_ref as lr
import nupc_ref as nr
import nupc_truepeak_ref as tr
from nupc_chain_ref import IN, OUT, STAGGERED
from test_gpu_nupc_chain import _blocks, _check, _taps
from test_gpu_nupc_limiter import EPS, FF, TOL, _code, _input, _reals

pytestmark = pytest.mark.gpu
H = tr.H
L1 = float(np.abs(tr.G).sum(axis=1).max())
ESTATE, EINVAL = -5, -1
SCHED = {16: ([16, 32], [2, 2]), 64: ([64, 128], [2, 2]), 2048: ([2048], [2])}
# L0 = 64 with D_e = 12 (the minimum), D = L0 and D > L0; L0 = 16: look-ahead and interpolator span several
# periods; L0 = 2048: two tiles, the 24 taps and the envelope's history cross the tile edge
SHAPES = [(64, 24), (64, 64), (64, 100), (16, 24), (16, 40), (2048, 24), (2048, 1024)]


def _mk(hip, rs, sched, n_out, taps="noise", gain=2.0, fmts=None, lim=None, groups=(), detector=tr.TRUE_PEAK, setup=None):
    """lim: (D, release) or None (the twin); groups: [(channels, threshold)]; fmts: a 4-byte format name per
    output (rs 4), default the convolver's float format; detector None: never selected"""
    dt = np.float32 if rs == 4 else np.float64
    nu = hip.Nupc(sched[0], sched[1], rs, 2, n_out)
    nu.set_interleaved(IN, FF[rs])
    nu.set_interleaved(OUT, FF[rs])
    if fmts:
        for c, name in enumerate(fmts):
            nu.set_format(OUT, c, hip.make_format(name, n_out, c * 4))
    rng = np.random.default_rng(7)
    for o in range(n_out):
        if taps == "noise":
            for i in range(2):
                nu.add_filter(i, o, _taps(rng, nu.taps, dt, 1)[0].astype(dt), out_scale=gain)
        else:
            nu.add_filter(o % 2, o, np.ones(1, dt), out_scale=gain)
    if setup:
        setup(nu)
    if lim:
        nu.enable_limiter(*lim)
        if detector is not None:
            nu.set_limiter_detector(detector)
            assert nu.limiter_detector() == detector
        for k, (chs, thr) in enumerate(groups):
            assert nu.add_limiter_group(chs, thr) == k
    nu.finalize()
    return nu


def _k(xr, chs, thr_min):
    """K of the module docstring for a group"""
    xm = np.abs(np.where(np.isfinite(xr[:, list(chs)]), xr[:, list(chs)], 0.0)).max()
    return 2 * H * 2.0 ** -52 * L1 * xm / thr_min


def _bars(tag, y, want, xd, rs, D, release, chs, K, ints=False, rms_bar=True):
    """the per-sample bar and the relative RMS bar of the module docstring on the channels chs -> the largest
    fraction of the per-sample bar.  rms_bar False: 16-bit outputs, whose rounding alone is above the RMS bar"""
    k = (max(release, 1) + D - H + 4) * EPS[8] + K + (2 * EPS[4] if rs == 4 else 0.0)
    top = 0.0
    for c in chs:
        fin = np.isfinite(want[:, c])
        assert np.array_equal(fin, np.isfinite(y[:, c])), c
        err = np.abs(y[fin, c] - want[fin, c])
        bar = k * np.abs(xd[fin, c]) + (1.0 if ints else 0.0)
        worst = (err / np.maximum(bar, 1e-300)).max()
        rms = cases.rel_rms(y[fin, c], want[fin, c])
        print("%s rs %d ch %d: worst error / bar %.3g, rel rms %.3g" % (tag, rs, c, worst, rms))
        assert np.all(err <= bar), (c, int((err - bar).argmax()), worst)
        assert rms <= TOL[rs] or not rms_bar, (c, rms)
        top = max(top, worst)
    return top


def _pair(hip, rs, sched, n_out, x, periods, **kw):
    """(twin's reals, limited convolver, its raw bytes, its status words): the same wiring and input through
    both; before(a, p) runs in front of the limited convolver's period p"""
    L0 = sched[0][0]
    lim, groups = kw.pop("lim"), kw.pop("groups")
    before = kw.pop("before", None)
    twin = _mk(hip, rs, sched, n_out, **{k: v for k, v in kw.items() if k in ("taps", "gain")})
    a = _mk(hip, rs, sched, n_out, lim=lim, groups=groups, **kw)
    assert a.limiter_delay() == lim[0] and a.L0 == L0
    xt, _ = _blocks(twin, x, L0, periods)
    ya, sts = _blocks(a, x, L0, periods, (lambda p: before(a, p)) if before else None)
    twin.close()
    return _reals(xt, rs, n_out), a, ya, sts


# ---------------------------------------------------------------- A. model match, sample ceiling, meter

@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("L0,D", SHAPES)
def test_model_match(hip, rs, L0, D):
    """noise with bursts, one group over outputs 0 and 1, output 2 in no group; the true-peak meter is read in
    the middle of the run and at its end: each reading covers the frames since the one before"""
    dt = np.float32 if rs == 4 else np.float64
    sched, release, thr = SCHED[L0], 50, 0.5
    periods = {16: 48, 64: 24, 2048: 3}[L0]
    x = _input(rs, L0, periods)
    groups = [((0, 1), thr)]
    half, first = periods // 2, []

    def before(a, p):
        if p == half:
            first.append(a.limiter_true_peak(0))
            assert a.limiter_true_peak(0) == 0.0                        # no block in between

    xr, a, ya, sts = _pair(hip, rs, sched, 3, x, periods, lim=(D, release), groups=groups, before=before)
    assert not any(sts)
    want, (s,), (meter,) = tr.limit_tp(xr, groups, [1.0] * 3, D, release, L0, dt)
    assert s.min() < 0.7 and (s[:len(s) // 3] < 1.0).any() and (s == 1.0).sum() < len(s)       # it did limit, early
    y = _reals(ya, rs, 3)
    _bars("A %d/%d" % (L0, D), y, want, lr.delayed(xr, D), rs, D, release, (0, 1), _k(xr, (0, 1), thr))
    assert np.abs(y[:, :2]).max() <= thr * (1 + (D - H + 4) * EPS[rs]) and np.abs(xr[:, :2]).max() > thr
    assert np.array_equal(y[D:, 2], xr[:-D, 2]) and not y[:D, 2].any() and xr[:, 2].any()      # untouched, D late
    got = first + [a.limiter_true_peak(0)]
    model = [meter[:half * L0].max(), meter[half * L0:].max()]
    bar = 2 * H * 2.0 ** -52 * L1 * np.abs(xr[:, :2]).max()
    print("A %d/%d rs %d: true-peak meter %s, model %s, sample peak %.6g" % (L0, D, rs, got, model, np.abs(xr[:, :2]).max()))
    assert abs(got[0] - model[0]) <= bar and abs(got[1] - model[1]) <= bar and model[0] != model[1]
    assert max(got) >= np.abs(xr[:, :2]).max()
    a.close()


# ---------------------------------------------------------------- B. the fs/4 sine, and sample-peak mode's bytes

@pytest.mark.parametrize("rs", [4, 8])
def test_fs4_sine(hip, rs):
    """amplitude 1, 45 degrees off the sampling instants, ceiling 0.8: the samples never reach the ceiling, the
    waveform does.  Sample-peak mode passes it untouched -- with the bytes of a convolver that never chose a
    detector -- and true-peak mode holds the true peak of its output at the ceiling"""
    dt = np.float32 if rs == 4 else np.float64
    L0, D, release, thr, periods = 64, 64, 4800, 0.8, 40
    sched = SCHED[L0]
    n = periods * L0
    sine = np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4)
    x = np.ascontiguousarray(np.stack([sine, 0.5 * sine], axis=1).astype(dt))
    groups = [((0, 1), thr)]
    xr, a, ya, _ = _pair(hip, rs, sched, 2, x, periods, taps="delta", gain=1.0, lim=(D, release), groups=groups)
    assert abs(np.abs(xr).max() - np.sqrt(0.5)) < 1e-6
    want, (s,), (meter,) = tr.limit_tp(xr, groups, [1.0, 1.0], D, release, L0, dt)
    y = _reals(ya, rs, 2)
    _bars("B", y, want, lr.delayed(xr, D), rs, D, release, (0, 1), _k(xr, (0, 1), thr))
    got = a.limiter_true_peak(0)
    tp_y = tr.detect(y[:, 0]).max()
    print("B rs %d: meter %.9f (sample peak %.5f), gain at least %.5f, true peak of y %.9f = 1 + %.3g ceilings"
          % (rs, got, np.abs(xr).max(), a.limiter_reduction(0), tp_y, tp_y / thr - 1))
    assert got > 1.2 * np.abs(xr).max() and abs(got - meter.max()) <= 2 * H * 2.0 ** -52 * L1 * np.abs(xr).max()
    # the model's 1e-5, and in T the roundings of y (2^-24 or 2^-53 each) through an interpolator of ||g||_1 < 2.21
    assert s.min() < 0.81 and tp_y <= thr * (1 + 1e-5 + 2 * EPS[rs]) and tp_y > 0.99 * thr
    a.close()
    # sample-peak mode: chosen explicitly or never chosen, the same bytes, and it never engages
    b = _mk(hip, rs, sched, 2, taps="delta", gain=1.0, lim=(D, release), groups=groups, detector=tr.SAMPLE_PEAK)
    c = _mk(hip, rs, sched, 2, taps="delta", gain=1.0, lim=(D, release), groups=groups, detector=None)
    yb, _ = _blocks(b, x, L0, periods)
    yc, _ = _blocks(c, x, L0, periods)
    assert yb.any() and np.array_equal(yb, yc) and c.limiter_detector() == tr.SAMPLE_PEAK
    ys = _reals(yb, rs, 2)
    assert np.array_equal(ys[D:], xr[:-D]) and b.limiter_reduction(0) == 1.0
    assert tr.detect(ys[:, 0]).max() > 1.2 * thr
    assert _code(b, lambda: b.limiter_true_peak(0)) == ESTATE
    b.close()
    c.close()


def test_sample_peak_mode_limits_with_the_same_bytes(hip):
    """noise that does limit: SAMPLE_PEAK chosen explicitly gives the bytes of a convolver that never chose"""
    rs, L0, periods = 8, 64, 24
    x = _input(rs, L0, periods)
    groups = [((0, 1), 0.5)]
    b = _mk(hip, rs, SCHED[L0], 2, lim=(24, 50), groups=groups, detector=tr.SAMPLE_PEAK)
    c = _mk(hip, rs, SCHED[L0], 2, lim=(24, 50), groups=groups, detector=None)
    yb, _ = _blocks(b, x, L0, periods)
    yc, _ = _blocks(c, x, L0, periods)
    assert np.array_equal(yb, yc) and b.limiter_reduction(0) == c.limiter_reduction(0) < 0.7
    b.close()
    c.close()


# ---------------------------------------------------------------- C. impulses across every boundary, non-finite x

@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("L0", [16, 64, 2048])
def test_impulses_at_the_boundaries(hip, rs, L0):
    """single impulses of 4 ceilings at frames L0 - 1, L0, 2 L0 + tile - 1 and 2 L0 + tile: the 24 taps that
    answer each straddle a period boundary or a tile edge"""
    dt = np.float32 if rs == 4 else np.float64
    D, release, thr, tile = 24, 48, 0.5, min(L0, 1024)
    periods = 4 + D // L0 + 1
    x = np.zeros((periods * L0, 2), dt)
    for k, at in enumerate((L0 - 1, L0, 2 * L0 + tile - 1, 2 * L0 + tile)):
        x[at, k % 2] = 2.0 * (-1) ** k
    groups = [((0, 1), thr)]
    xr, a, ya, _ = _pair(hip, rs, SCHED[L0], 2, x, periods, taps="delta", gain=1.0, lim=(D, release), groups=groups)
    assert (np.abs(xr) > 1.9).sum() == 4
    want, (s,), _ = tr.limit_tp(xr, groups, [1.0, 1.0], D, release, L0, dt)
    y = _reals(ya, rs, 2)
    _bars("C %d" % L0, y, want, lr.delayed(xr, D), rs, D, release, (0, 1), _k(xr, (0, 1), thr))
    assert np.abs(y).max() <= thr * (1 + (D - H + 4) * EPS[rs]) and np.abs(y).max() > 0.9 * thr
    a.close()


@pytest.mark.parametrize("rs", [4, 8])
def test_non_finite_samples(hip, rs):
    """a NaN and an Inf input sample: the transforms spread each over the frames its partitions reach.  The
    quantiser reports a non-finite real in the period's status word (bit 0) and writes nothing for it, in the
    twin as in the limited convolver, so such a sample shows what its place in the period buffer held before.
    The input is silent for four periods in front of either sample: the buffers hold zeros there, the twin's
    bytes show 0 for a non-finite x -- what it contributes to the detector -- and the model applies as it
    stands, to the limited convolver's unwritten samples too"""
    dt = np.float32 if rs == 4 else np.float64
    L0, D, release, thr, periods = 64, 40, 50, 0.5, 24
    sched = ([64], [2])
    x = _input(rs, L0, periods)
    x[1 * L0:5 * L0] = 0.0
    x[10 * L0:14 * L0] = 0.0
    x[5 * L0 + 3, 0] = np.nan
    x[14 * L0 + 60, 1] = np.inf
    groups = [((0, 1), thr)]
    twin = _mk(hip, rs, sched, 2)
    a = _mk(hip, rs, sched, 2, lim=(D, release), groups=groups)
    xt, st_t = _blocks(twin, x, L0, periods)
    ya, st_a = _blocks(a, x, L0, periods)
    bad_t = [p for p in range(periods) if st_t[p] & 1]
    bad_a = [p for p in range(periods) if st_a[p] & 1]
    xr = _reals(xt, rs, 2)
    gone = ~xr.any(axis=1)
    print("C nan rs %d: periods with a non-finite real: twin %s, limited %s; silent frames per period %s"
          % (rs, bad_t, bad_a, gone.reshape(periods, L0).sum(axis=1)))
    assert bad_t and bad_t[0] == 5 and 14 in bad_t and len(bad_t) <= 8 and bad_a and bad_a[0] >= 5
    assert np.all(np.isfinite(xr)) and gone[5 * L0:8 * L0].sum() >= L0 and gone[14 * L0:17 * L0].sum() >= L0
    want, (s,), (meter,) = tr.limit_tp(xr, groups, [1.0, 1.0], D, release, L0, dt)
    assert s.min() < 0.7 and s[-3 * L0:].min() < 1.0
    y = _reals(ya, rs, 2)
    _bars("C nan", y, want, lr.delayed(xr, D), rs, D, release, (0, 1), _k(xr, (0, 1), thr))
    got = a.limiter_true_peak(0)
    assert np.isfinite(got) and abs(got - meter.max()) <= 2 * H * 2.0 ** -52 * L1 * np.abs(xr).max()
    a.close()
    twin.close()


# ---------------------------------------------------------------- D. idle exactness

@pytest.mark.parametrize("rs,outfmt", [(4, None), (8, None), (4, "S24_4LE")])
def test_idle_exactness(hip, rs, outfmt):
    """below the ceiling between the samples too: the twin's bytes, D frames later"""
    L0, D, periods = 64, 40, 24
    x = _input(rs, L0, periods, amp=0.02, bursts=False)
    fm = [outfmt] * 2 if outfmt else None
    twin = _mk(hip, rs, SCHED[L0], 2, fmts=fm)
    a = _mk(hip, rs, SCHED[L0], 2, fmts=fm, lim=(D, 500), groups=[((0, 1), 0.999)])
    xt, _ = _blocks(twin, x, L0, periods)
    ya, _ = _blocks(a, x, L0, periods)
    fb = len(xt) // (periods * L0)
    xt, ya = xt.reshape(-1, fb), ya.reshape(-1, fb)
    assert xt.any() and np.array_equal(ya[D:], xt[:-D])
    assert a.limiter_reduction(0) == 1.0 and 0.0 < a.limiter_true_peak(0) < 0.999
    a.close()
    twin.close()


# ---------------------------------------------------------------- E. groups of 1, 2 and 8, mixed formats

def test_groups_and_mixed_formats(hip):
    """float32, 12 outputs on 4-byte frames: {0} S32, {1, 2} float and S24, {3 .. 10} all three kinds, 11 in no
    group.  Thresholds are fractions of full scale, x is in output units"""
    rs, L0, D, release, periods = 4, 64, 40, 50, 24
    names = ["S32_LE", "FLOAT_LE", "S24_4LE"] + ["FLOAT_LE", "S32_LE", "S24_4LE"] * 2 + ["S32_LE", "S24_4LE", "FLOAT_LE"]
    fmts = [bo.make_format(nm, 12, c * 4) for c, nm in enumerate(names)]
    scale = np.array([f.scale for f in fmts])
    groups = [((0,), 0.5), ((1, 2), 0.4), (tuple(range(3, 11)), 0.6)]
    x = _input(rs, L0, periods)
    twin = _mk(hip, rs, SCHED[L0], 12)
    a = _mk(hip, rs, SCHED[L0], 12, fmts=names, lim=(D, release), groups=groups)
    xt, _ = _blocks(twin, x, L0, periods)
    ya, _ = _blocks(a, x, L0, periods)
    xr = _reals(xt, rs, 12) / scale                                     # output units: exact, the scales are powers of 2
    want, env, meter = tr.limit_tp(xr, groups, scale, D, release, L0, np.float32)
    got = nr.ints(ya, fmts, periods * L0)
    xd = lr.delayed(xr, D)
    for g, (chs, thr) in enumerate(groups):
        assert env[g].min() < 0.8
        K = max(_k(xr[:, [c]] * scale[c], (0,), thr) for c in chs)
        for kind in (False, True):
            sel = [c for c in chs if (not fmts[c].isfloat) == kind]
            if sel:
                _bars("E g%d" % g, got, want, xd, rs, D, release, sel, K, ints=kind)
        tp = a.limiter_true_peak(g)
        assert abs(tp - meter[g].max()) <= 2 * H * 2.0 ** -52 * L1 * meter[g].max() and tp > thr
    assert np.array_equal(got[D:, 11], xr[:-D, 11])
    assert not np.array_equal(env[0], env[1]) and not np.array_equal(env[1], env[2])
    a.close()
    twin.close()


def test_full_group_float64(hip):
    rs, L0, D, release, periods = 8, 64, 24, 50, 16
    groups = [((4,), 0.5), ((0, 2), 0.5), ((1, 3, 5, 6, 7, 8, 9, 10), 0.5)]
    x = _input(rs, L0, periods)
    xr, a, ya, _ = _pair(hip, rs, SCHED[L0], 11, x, periods, lim=(D, release), groups=groups)
    want, env, _ = tr.limit_tp(xr, groups, [1.0] * 11, D, release, L0)
    y = _reals(ya, rs, 11)
    _bars("E8", y, want, lr.delayed(xr, D), rs, D, release, range(11), _k(xr, range(11), 0.5))
    a.close()


# ---------------------------------------------------------------- F. run-time thresholds

@pytest.mark.parametrize("rs", [4, 8])
def test_runtime_thresholds(hip, rs):
    dt = np.float32 if rs == 4 else np.float64
    L0, D, release, periods = 64, 40, 500, 48
    plan = {12: 0.5, 24: 0.25, 36: float("inf")}
    thr, cur = [], float("inf")
    for p in range(periods):
        cur = plan.get(p, cur)
        thr.append(cur)
    x = _input(rs, L0, periods)
    box = []

    def before(p):
        if p in plan:
            box[0].set_limiter_threshold(0, plan[p])

    twin = _mk(hip, rs, SCHED[L0], 2)
    a = _mk(hip, rs, SCHED[L0], 2, lim=(D, release), groups=[((0, 1), float("inf"))])
    box.append(a)
    xt, _ = _blocks(twin, x, L0, periods)
    ya, _ = _blocks(a, x, L0, periods, before)
    xr, y = _reals(xt, rs, 2), _reals(ya, rs, 2)
    want, (s,), _ = tr.limit_tp(xr, [((0, 1), thr)], [1.0, 1.0], D, release, L0, dt)
    assert np.all(s[:12 * L0] == 1.0) and s[12 * L0:24 * L0].min() < 0.8 and s[24 * L0:36 * L0].min() < s[12 * L0:24 * L0].min()
    _bars("F", y, want, lr.delayed(xr, D), rs, D, release, (0, 1), _k(xr, (0, 1), 0.25))
    a.close()
    twin.close()


# ---------------------------------------------------------------- G. whole chain, the dither path

def test_dither_instantiation_float32(hip):
    """float32, three S16 outputs, HP-TPDF dither on output 0, which is in no group: the DITHER instantiation of
    the limit kernel runs for every channel.  Outputs 1 and 2, one group, go through its detector, envelope and
    plain quantiser and are held to the model in counts.  The dithered channel itself is compared in
    test_whole_chain, in float64: its quantiser feeds its error back, so a float32 run departs from a float64
    model by more than a count"""
    rs, L0, D, release, periods, thr = 4, 64, 40, 50, 24, 0.5
    groups = [((1, 2), thr)]

    def setup(nu):
        nu.set_interleaved(OUT, "S16_LE")
        nu.enable_dither([0], 300)

    x = _input(rs, L0, periods)
    twin = _mk(hip, rs, SCHED[L0], 3)
    a = _mk(hip, rs, SCHED[L0], 3, lim=(D, release), groups=groups, setup=setup)
    xt, _ = _blocks(twin, x, L0, periods)
    ya, _ = _blocks(a, x, L0, periods)
    fm = bo.interleaved_formats("S16_LE", 3)
    xr = _reals(xt, rs, 3) * 32768.0                                    # output units
    want, (s,), _ = tr.limit_tp(xr, groups, [2.0 ** -15] * 3, D, release, L0, np.float32)
    got = nr.ints(ya, fm, periods * L0)
    assert s.min() < 0.7 and got[:, 0].any()
    _bars("G32", got, want, lr.delayed(xr, D), rs, D, release, (1, 2), _k(xr / 32768.0, (1, 2), thr), ints=True, rms_bar=False)
    assert np.abs(got[:, 1:]).max() <= thr * 32768 + 1
    a.close()
    twin.close()


def test_whole_chain(hip):
    """test_gpu_nupc_limiter.test_whole_chain in true-peak mode: the limiter behind the sub-delay FIR of output 1,
    HP-TPDF dither on output 0 (S16: the DITHER instantiation), an output-gain ramp from 1 to 6 that drives the
    group into limiting, a staggered cross-faded switch, an integer output delay and a mute"""
    rs, sched, D, release = 8, ([64, 128, 256, 512], [2, 2, 2, 6]), 64, 500
    L0 = sched[0][0]
    dt = np.float32 if rs == 4 else np.float64
    ch = tr.LimitedChainTP(sched, rs, 2, 2, FF[rs], "S16_LE", half=15, dither=(0,))
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
    nu.set_limiter_detector(tr.TRUE_PEAK)
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
    tp = nu.limiter_true_peak(0)
    print("G: true-peak meter %.17g, model %.17g" % (tp, ch.true_peak[0].max()))
    # the chain's bar is an RMS one (3 TOL per block); a single peak gets a crest allowance of 30 on top
    assert abs(tp - ch.true_peak[0].max()) <= 100 * TOL[rs] * tp
    nu.close()


# ---------------------------------------------------------------- H. errors on a live handle

def test_state_and_argument_errors(hip):
    L = hip.lib()
    nu = hip.Nupc([64], [2], 4, 2, 3)
    for o in range(3):
        nu.add_filter(0, o, np.ones(8, np.float32))
    assert nu.limiter_detector() == tr.SAMPLE_PEAK
    assert _code(nu, lambda: nu.set_limiter_detector(tr.TRUE_PEAK)) == ESTATE       # before enable_limiter
    nu.enable_limiter(23, 50.0)
    assert _code(nu, lambda: nu.set_limiter_detector(tr.TRUE_PEAK)) == EINVAL       # D = 23 < 2 H
    assert "24" in L.bfhip_nupc_last_error().decode() and nu.limiter_detector() == tr.SAMPLE_PEAK
    nu.set_limiter_detector(tr.SAMPLE_PEAK)
    for bad in (2, -1, 7):
        assert _code(nu, lambda: nu.set_limiter_detector(bad)) == EINVAL, bad
    assert nu.add_limiter_group([0, 1], 0.5) == 0
    assert _code(nu, lambda: nu.limiter_true_peak(0)) == ESTATE                      # sample-peak mode
    assert _code(nu, lambda: nu.limiter_true_peak(1)) == EINVAL
    nu.close()
    nu = hip.Nupc([64], [2], 4, 2, 3)
    for o in range(3):
        nu.add_filter(0, o, np.ones(8, np.float32))
    nu.enable_limiter(24, 50.0)
    nu.set_limiter_detector(tr.TRUE_PEAK)                                           # D = 24 is accepted
    nu.set_limiter_detector(tr.SAMPLE_PEAK)
    nu.set_limiter_detector(tr.TRUE_PEAK)
    assert nu.limiter_detector() == tr.TRUE_PEAK and nu.limiter_delay() == 24
    assert nu.add_limiter_group([0, 1], 0.5) == 0
    v = C.c_double(-3.0)
    assert L.bfhip_nupc_get_limiter_true_peak(nu.h, 1, C.byref(v)) == EINVAL and v.value == -3.0
    assert L.bfhip_nupc_get_limiter_true_peak(nu.h, -1, C.byref(v)) == EINVAL
    assert L.bfhip_nupc_get_limiter_true_peak(nu.h, 0, None) == EINVAL
    assert nu.limiter_true_peak(0) == 0.0                                           # nothing detected yet
    nu.finalize()
    assert _code(nu, lambda: nu.set_limiter_detector(tr.SAMPLE_PEAK)) == ESTATE     # after finalize
    assert nu.limiter_detector() == tr.TRUE_PEAK and nu.limiter_true_peak(0) == 0.0
    st, y = nu.block(np.full((64, 2), 0.25, np.float32))
    assert st == 0 and nu.limiter_true_peak(0) > 0.0 and nu.limiter_true_peak(0) == 0.0
    nu.close()


# ---------------------------------------------------------------- I. allocation faults (the state's size changed)

def test_every_allocation_failure_is_an_error_code(hip):
    """create ... finalize ... blocks ... destroy of a true-peak convolver with the n-th allocation failing, n =
    1, 2, ... until a life no longer reaches the armed allocation"""
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
            nu.set_limiter_detector(tr.TRUE_PEAK)
            nu.add_limiter_group([0, 2], 0.5)
            nu.finalize()
            return np.concatenate([nu.block(x)[1] for _ in range(3)])
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
            break
        absorbed += 1
        assert np.array_equal(got, want)
    print("I: %d allocations walked, %d errors, %d absorbed" % (n - 1, errors, absorbed))
    assert errors + absorbed == n - 1 and errors >= 19 and absorbed <= 6
    assert np.array_equal(life(), want) and want.any()
