"""CPU: the float64 model of the equaliser render (tests/eq_ref.py) that the device tests compare
against.  A flat curve of magnitude 1 and phase 0 is a unit pulse at tap R/2, and the sign form
(-1)^n cos(phi), the specification, differs from the reference's literal cos(-R pi f + phi) by the
rounding of that argument only."""
import numpy as np
import pytest

import cases
import eq_ref


@pytest.mark.parametrize("R", [64, 4096, 32768])
def test_flat_curve_is_a_unit_pulse_at_the_middle_tap(R):
    taps = eq_ref.render(R, *eq_ref.flat())
    want = np.zeros(R)
    want[R // 2] = 1.0
    off = np.abs(taps - want).max()
    print("R %d: largest deviation from the pulse %.3g" % (R, off))
    assert off <= 1e-12


@pytest.mark.parametrize("R", [64, 4096, 32768])
def test_sign_form_is_the_literal_form_up_to_argument_rounding(R):
    """the argument -R pi f reaches pi R/2 in magnitude, so its float64 rounding is up to
    pi (R/2) 2^-53 rad, and a phase error of e rad moves a bin by e relative: that is the bound"""
    bound = np.pi * (R / 2) * 2.0 ** -53
    for seed in range(4):
        curve = eq_ref.random_bands(32, 100 + seed)
        got = cases.rel_rms(eq_ref.render_literal(R, *curve), eq_ref.render(R, *curve))
        print("R %d seed %d: rel rms %.3g (bound %.3g)" % (R, seed, got, bound))
        assert got <= bound
