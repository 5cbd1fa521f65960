"""CPU: the float64 model of the look-ahead peak limiter (tests/nupc_limiter_ref.py) has the two properties
the header states, and the library's frame-by-frame evaluation (bfhip_selftest_limiter_envelope, host code
that needs no device) agrees with it.

    ceiling          s[t] <= r[t - D] + (D + 2) 2^-52: the box sum of D + 1 terms, none above r[t - D], rounds
                     once per term
    idle exactness   input below the threshold: s == 1.0 and y[D:] == x[:-D], bit for bit
    selftest         the bar of the device's float64 envelope, (R + D + 4) 2^-52 with R = max(release, 1)
                     (both sides walk the frames one by one, so they agree far inside it)"""
import numpy as np
import pytest

import brutefir_amd as bf
import nupc_limiter_ref as lr

DS = (1, 16, 64, 96)
RELEASES = (0, 50, 4800)


def _p(seed, n, D):
    """noise around 0.3 of the threshold with bursts of x12 for 40 frames, one inside the first D frames"""
    rng = np.random.default_rng(seed)
    p = np.abs(rng.standard_normal(n)) * 0.3
    for at in (0, 777, 2000, 2040, 3500):
        p[at:at + 40] *= 12.0
    return p


@pytest.mark.parametrize("release", RELEASES)
@pytest.mark.parametrize("D", DS)
def test_ceiling(D, release):
    n = 6000
    p = _p(D + release, n, D)
    r, m, e, s = lr.envelope_parts(p, D, release)
    assert (p > 1).sum() > 100 and s.min() < 0.5
    assert np.all(e <= m) and np.all(m <= r)
    rd = np.concatenate([np.ones(D), r[:n - D]])
    over = s - rd
    print("D %d release %d: s - r[t - D] at most %.3g" % (D, release, over.max()))
    assert over.max() <= (D + 2) * 2.0 ** -52
    # and through limit(): |y| <= ceil (1 + (D + 4) eps) in both real types
    x = (p * np.sign(np.sin(np.arange(n)))).astype(np.float32).astype(np.float64)[:, None] * 0.5
    for dt, eps in ((np.float32, 2.0 ** -23), (np.float64, 2.0 ** -52)):
        y, _ = lr.limit(x, [((0,), 0.5)], [1.0], D, release, 50, dt)
        assert np.abs(y).max() <= 0.5 * (1 + (D + 4) * eps)
        assert np.abs(y).max() > 0.49


@pytest.mark.parametrize("release", RELEASES)
@pytest.mark.parametrize("D", DS)
def test_idle_exactness(D, release):
    rng = np.random.default_rng(D)
    n = 3000
    x = rng.standard_normal((n, 3)) * 0.02
    x[5, 1] = np.nan                                   # contributes nothing, arrives as it is
    x[9, 0] = 0.999 / 2.0                              # exactly at the ceiling: p == 1 is not above it
    y, env = lr.limit(x, [((0, 1), 0.999), ((2,), np.inf)], [2.0, 2.0, 1.0], D, release, 100)
    for s in env:
        assert np.all(s == 1.0)
    assert np.array_equal(y[D:], x[:-D], equal_nan=True) and not y[:D].any()


@pytest.mark.parametrize("release", RELEASES)
@pytest.mark.parametrize("D", DS)
def test_selftest_equals_the_model(D, release):
    p = _p(3 * D + release, 5000, D)
    p[100] = np.inf
    p[101] = np.nan
    want = lr.envelope(p, D, release)
    got = bf.limiter_envelope(D, release, p)
    err = np.abs(got - want).max()
    print("D %d release %d: selftest - model at most %.3g" % (D, release, err))
    assert err <= (max(release, 1) + D + 4) * 2.0 ** -52


def test_thresholds_by_period():
    """a threshold applies to the frames of its period; they leave D frames later"""
    L0, D = 32, 8
    x = np.full((4 * L0, 1), 0.8)
    y, (s,) = lr.limit(x, [((0,), [np.inf, 0.4, 0.4, np.inf])], [1.0], D, 0, L0)
    assert np.all(s[:L0] == 1.0) and np.all(s[L0 + D:3 * L0] == 0.5) and np.all(s[3 * L0 + 2 * D:] == 1.0)
    assert np.all(s[L0:L0 + D] < 1.0)                  # the look-ahead: the gain is down before the loud frame leaves
    assert np.abs(y[L0 + D:3 * L0 + D]).max() <= 0.4
