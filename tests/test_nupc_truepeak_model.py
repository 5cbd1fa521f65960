"""CPU: the float64 model of the limiter's true-peak detector (tests/nupc_truepeak_ref.py) against the library's
host definition (bfhip_selftest_truepeak_filter, bfhip_selftest_truepeak: no device) and against the properties
the header states.

    taps, detector   model and library compute the same formulas in float64: a few ulp apart (libm against
                     numpy in sin, sqrt and the I0 series; the 24-term sums may be contracted to fma on one side)
    phase 0          the sample itself, H frames late: exact
    interpolation    sines at 13 phases: <= 2e-4 of the amplitude up to 0.35 fs, <= 3e-3 at 0.40 fs (twice the
                     figures of the header)
    fs/4 sine        45 degrees off the sampling instants, amplitude 1, ceiling 0.8: the sample-peak limiter never
                     engages (true peak of its output above 1.2 ceilings), the true-peak limiter holds
                     ceiling (1 + 1e-5) over the whole run (measured: 1 + 4.4e-7)
    sample ceiling   |y| <= ceil (1 + (D_e + 4) eps) and idle exactness, on random signals
    overshoot        the true peak of y over seeded noise bursts, printed; asserted only below 1.05 (measured: 1.0104)"""
import numpy as np
import pytest

import brutefir_amd as bf
import nupc_limiter_ref as lr
import nupc_truepeak_ref as tr

H = tr.H


def test_taps_equal_the_selftest():
    got = bf.truepeak_filter()
    err = np.abs(got - tr.G)
    bar = 8 * 2.0 ** -52 * np.maximum(np.abs(tr.G), 2.0 ** -10)        # sin(pi v) near a zero of the sinc: absolute
    print("taps: worst error / bar %.3g; sum |g| per phase %s" % ((err / bar).max(), np.abs(got).sum(axis=1)))
    assert np.all(err <= bar)
    assert got.shape == (3, 2 * H) and np.allclose(got[0], got[2][::-1], rtol=0, atol=1e-15)    # q and 4 - q mirror
    assert abs(got[1][H - 1] - got[1][H]) < 1e-15 and 0.6 < got[1][H] < 0.64                     # the half-sample pair


def test_detect_equals_the_selftest():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(3000)
    x[100], x[200], x[201] = np.nan, np.inf, -np.inf
    want, got = tr.detect(x), bf.truepeak(x)
    l1 = np.abs(tr.G).sum(axis=1).max()
    bar = 2 * H * 2.0 ** -52 * l1 * np.abs(x[np.isfinite(x)]).max()
    print("detect: selftest - model at most %.3g, bar %.3g" % (np.abs(got - want).max(), bar))
    assert np.all(np.isfinite(got)) and np.abs(got - want).max() <= bar
    assert bf.lib().bfhip_selftest_truepeak(-1, None, None) == -1
    assert bf.lib().bfhip_selftest_truepeak_filter(None) == -1
    assert len(bf.truepeak(np.zeros(0))) == 0


def test_phase_0_is_exact():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(500)
    x[7] = np.nan
    u = tr.phases(x)
    want = np.concatenate([np.zeros(H), np.where(np.isfinite(x), x, 0.0)[:-H]])
    assert np.array_equal(u[:, 0], want)
    assert np.all(tr.detect(x) >= np.abs(want)) and np.all(bf.truepeak(x) >= np.abs(want))     # never below the sample peak


@pytest.mark.parametrize("f,bar", [(0.01, 2e-4), (0.1, 2e-4), (0.25, 2e-4), (0.35, 2e-4), (0.40, 3e-3)])
def test_interpolation_error_on_sines(f, bar):
    n = 400
    t = np.arange(n, dtype=np.float64)
    worst = 0.0
    for ph in np.arange(13) * (2 * np.pi / 13):
        u = tr.phases(np.sin(2 * np.pi * f * t + ph))
        for q in range(4):
            want = np.sin(2 * np.pi * f * (t - H + q / 4.0) + ph)
            worst = max(worst, np.abs(u[2 * H:, q] - want[2 * H:]).max())           # behind the start-up transient
    print("f = %.2f fs: interpolation error at most %.3g" % (f, worst))
    assert worst <= bar


def _fs4(n, amp=1.0):
    return amp * np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4)


def test_fs4_sine_sample_peak_misses_true_peak_holds():
    D, release, ceil, n, L0 = 64, 4800, 0.8, 9600, 64
    x = _fs4(n)[:, None]
    assert abs(np.abs(x).max() - np.sqrt(0.5)) < 1e-12
    y_s, (s_s,) = lr.limit(x, [((0,), ceil)], [1.0], D, release, L0)
    tp_s = tr.detect(y_s[:, 0]).max()
    print("fs/4 sine through the sample-peak model: sample peak %.5f, true peak %.5f = %.4f ceilings"
          % (np.abs(y_s).max(), tp_s, tp_s / ceil))
    assert np.all(s_s == 1.0) and tp_s > 1.2 * ceil
    y_t, (s_t,), (meter,) = tr.limit_tp(x, [((0,), ceil)], [1.0], D, release, L0)
    tp_t = tr.detect(y_t[:, 0]).max()
    print("through the true-peak model: true peak %.9f = 1 + %.3g ceilings, smallest gain %.5f, meter %.5f"
          % (tp_t, tp_t / ceil - 1, s_t.min(), meter.max()))
    assert tp_t <= ceil * (1 + 1e-5) and tp_t > 0.99 * ceil
    # behind the onset (a sine that starts at full level is broadband there) the reading is the sine's amplitude
    assert abs(meter[200:].max() - 1.0) < 2e-4 and meter.max() < 1.02 and ceil / 1.02 < s_t.min() < ceil


@pytest.mark.parametrize("release", [0, 48, 4800])
@pytest.mark.parametrize("D", [24, 64, 100])
def test_sample_ceiling_and_idle_exactness(D, release):
    rng = np.random.default_rng(D + release)
    n, De = 6000, D - H
    x = rng.standard_normal((n, 2)) * 0.3
    for at in (0, 777, 2000, 2040, 3500):
        x[at:at + 40] *= 12.0
    x = x.astype(np.float32).astype(np.float64)
    for dt, eps in ((np.float32, 2.0 ** -23), (np.float64, 2.0 ** -52)):
        y, (s,), _ = tr.limit_tp(x, [((0, 1), 0.5)], [1.0, 1.0], D, release, 50, dt)
        assert s.min() < 0.5 and np.abs(y).max() <= 0.5 * (1 + (De + 4) * eps)
    # idle: below the ceiling between the samples too
    quiet = rng.standard_normal((n, 3)) * 0.02
    quiet[5, 1] = np.nan
    y, env, meter = tr.limit_tp(quiet, [((0, 1), 0.999), ((2,), np.inf)], [2.0, 2.0, 1.0], D, release, 100)
    for s in env:
        assert np.all(s == 1.0)
    assert np.array_equal(y[D:], quiet[:-D], equal_nan=True) and not y[:D].any()
    assert np.all(np.isfinite(meter[0])) and meter[0].max() < 0.999


@pytest.mark.parametrize("release", [0, 48, 4800])
def test_true_peak_overshoot_on_noise_bursts(release):
    """recorded, not a guarantee: while s moves across the interpolator's span the bound is approximate"""
    D, ceil, L0 = 64, 0.5, 64
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        x = rng.standard_normal((40 * L0, 1)) * 0.05
        at = 10 * L0 + int(rng.integers(0, L0))
        x[at:at + 200] *= 30.0
        y, (s,), _ = tr.limit_tp(x, [((0,), ceil)], [1.0], D, release, L0)
        assert s.min() < 0.5
        worst = max(worst, tr.detect(y[:, 0]).max() / ceil)
    print("release %d: true peak of y over 20 noise bursts at most %.4f ceilings" % (release, worst))
    assert worst < 1.05
