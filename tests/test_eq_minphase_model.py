"""CPU: the float64 model of the minimum-phase equaliser render (tests/eq_minphase_ref.py) that the
device tests compare against.  A flat curve is a unit pulse at tap 0; the magnitude response of the
taps is the curve's M, the linear render's; the energy sits at the first taps, where the linear
render (tests/eq_ref.py) has it around tap R/2; and the total energy of the two renders is the same
(equal magnitudes, Parseval)."""
import functools

import numpy as np
import pytest

import eq_minphase_ref
import eq_ref

CURVES = {"7 bands": eq_ref.random_bands(7, 1), "130 bands": eq_ref.random_bands(130, 2)}


def _zero_phase(curve):
    return curve[0], curve[1], [0.0] * len(curve[0])


@functools.lru_cache(maxsize=None)
def _min(R, name, zero_phase):
    c = CURVES[name]
    taps = eq_minphase_ref.render(R, *(_zero_phase(c) if zero_phase else c))
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def _lin(R, name):
    taps = eq_ref.render(R, *_zero_phase(CURVES[name]))
    taps.setflags(write=False)
    return taps


@pytest.mark.parametrize("R", [64, 4096, 32768])
def test_flat_curve_is_a_unit_pulse_at_tap_0(R):
    taps = eq_minphase_ref.render(R, *eq_ref.flat())
    want = np.zeros(R)
    want[0] = 1.0
    off = np.abs(taps - want).max()
    print("R %d: largest deviation from the pulse %.3g" % (R, off))
    assert off <= 1e-12


@pytest.mark.parametrize("R", [64, 16384, 65536])
@pytest.mark.parametrize("zero_phase", [False, True], ids=["own phases", "zero phases"])
@pytest.mark.parametrize("name", list(CURVES))
def test_magnitude_response_is_the_curve(name, zero_phase, R):
    M, _ = eq_minphase_ref.curve(R, *CURVES[name])
    off = np.abs(np.abs(np.fft.rfft(_min(R, name, zero_phase))) / M - 1.0).max()
    print("R %d %s: max | |rfft(taps)| / M - 1 | %.3g" % (R, name, off))
    assert off <= 1e-12


@pytest.mark.parametrize("R", [16384, 65536])
@pytest.mark.parametrize("name", list(CURVES))
def test_energy_sits_at_the_first_taps(name, R):
    taps, lin = _min(R, name, True), _lin(R, name)
    head = np.sum(taps[:R // 8] ** 2) / np.sum(taps ** 2)
    print("R %d %s: largest tap %d, energy in the first R/8 taps %.6f; linear render's largest tap %d"
          % (R, name, np.argmax(np.abs(taps)), head, np.argmax(np.abs(lin))))
    assert np.argmax(np.abs(taps)) == 0
    assert head >= 0.99
    assert np.argmax(np.abs(lin)) == R // 2


@pytest.mark.parametrize("R", [16384, 65536])
@pytest.mark.parametrize("name", list(CURVES))
def test_total_energy_is_the_linear_renders(name, R):
    e_min, e_lin = np.sum(_min(R, name, True) ** 2), np.sum(_lin(R, name) ** 2)
    print("R %d %s: energy %.17g, linear %.17g" % (R, name, e_min, e_lin))
    assert abs(e_min - e_lin) <= 1e-12 * e_lin
