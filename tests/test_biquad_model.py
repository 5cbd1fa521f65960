"""The float64 model of the section render (tests/biquad_ref.py) against an independent truth: the plain
direct-form recursion.

OWN renders taps[t] = sum_m h[t + m R], the cascade's impulse response time-aliased at R: the recursion's
response of K R samples folded to R must agree, K doubled until the last R/2 samples are below 1e-17 of
the peak.  Bound 1e-12 relative RMS: the two sides share nothing but the coefficients; measured
3.6e-15 (`tone`) and 1.4e-14 .. 1.5e-14 (`mixed`).  `room` is left out of that one test: with poles 1e-4 from the unit circle the
recursion itself is only good to about 5e-13 there.  No device and no library."""
import numpy as np
import pytest

import biquad_ref
import cases

SETS = biquad_ref.sets()


def _folded_impulse(sections, R):
    K = 2
    while True:
        h = biquad_ref.impulse(sections, K * R)
        if np.abs(h[-R // 2:]).max() < 1e-17 * np.abs(h).max():
            return h.reshape(K, R).sum(axis=0), K
        K *= 2
        assert K * R <= 1 << 22, "the response does not decay"


@pytest.mark.parametrize("name,R", [("tone", 4096), ("tone", 16384), ("mixed", 64), ("mixed", 1024), ("mixed", 8192)])
def test_own_render_is_the_time_aliased_recursion(name, R):
    want, K = _folded_impulse(SETS[name], R)
    err = cases.rel_rms(biquad_ref.render(R, SETS[name], "own"), want)
    print("%s R %d (K %d): rel rms %.3g (limit 1e-12)" % (name, R, K, err))
    assert err <= 1e-12


@pytest.mark.parametrize("R", [8, 64, 4096])
def test_flat_is_a_unit_pulse(R):
    pulse = np.zeros(R)
    pulse[0] = 1.0
    assert np.abs(biquad_ref.render(R, SETS["flat"], "own") - pulse).max() <= 1e-15
    assert np.abs(biquad_ref.render(R, SETS["flat"], "linear") - np.roll(pulse, R // 2)).max() <= 1e-15


@pytest.mark.parametrize("name", ["tone", "mixed", "room", "many"])
def test_linear_render_is_symmetric_about_the_middle(name):
    R = 1024
    t = biquad_ref.render(R, SETS[name], "linear")
    assert np.abs(t[1:] - t[1:][::-1]).max() <= 1e-13 * np.abs(t).max()       # t[R/2 + d] == t[R/2 - d]
    assert abs(np.argmax(np.abs(t)) - R // 2) <= 1


def test_every_shared_set_is_stable():
    for name, s in SETS.items():
        assert s.shape[1] == 5 and biquad_ref.stable(s), name
    assert len(SETS["many"]) == 32 and len(SETS["mixed"]) == 7
    assert not biquad_ref.stable([1, 0, 0, 0, 1.0]) and not biquad_ref.stable([1, 0, 0, 1.5, 0.5])
    assert not biquad_ref.stable([1, 0, 0, float("nan"), 0])
