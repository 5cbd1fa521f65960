"""CPU: the float64 model of the BS.1770 loudness meter (tests/loudness_ref.py) and the host definition
(csrc/loudness_host.h through the bfhip_selftest_* calls) against the standard: the coefficient table of
BS.1770-4 at 48 kHz, its 997 Hz calibration (-3.01 LUFS), EBU Tech 3341's -23 LUFS stereo sine within 0.1 LU,
the gate on a -40 / -20 / silence programme, and the two implementations against each other."""
import math

import numpy as np
import pytest

import brutefir_amd as bf
import loudness_ref as lr

# ITU-R BS.1770-4, tables 1 and 2
SHELF_B = (1.53512485958697, -2.69169618940638, 1.19839281085285)
SHELF_A = (-1.69065929318241, 0.73248077421585)
HP_A = (-1.99004745483398, 0.99007225036621)


def test_coefficients_at_48000_are_the_standards():
    c = lr.kweighting(48000)
    want = SHELF_B + SHELF_A + (1.0, -2.0, 1.0) + HP_A
    err = np.abs(c - np.array(want)).max()
    print("coefficients at 48000: worst |error| %.3g (bar 1e-13)" % err)
    assert err <= 1e-13


@pytest.mark.parametrize("fs", [8000, 44100, 48000, 192000])
def test_host_design_matches_the_model(fs):
    got, want = bf.kweighting(fs), lr.kweighting(fs)
    err = np.abs(got / want - 1.0).max()
    print("fs %d: worst relative error %.3g (bar 1e-15)" % (fs, err))
    assert err <= 1e-15


@pytest.fixture(scope="module")
def sine48():
    """5 s of a 997 Hz sine at full scale, fs 48000, and its sub-block energies (weight 1)"""
    v = lr.sine(48000, 5.0)
    return v, lr.channel_energy(v, 48000)


def test_calibration_sine(sine48):
    """BS.1770: a 997 Hz sine at full scale in one channel reads -3.01 LUFS"""
    _, E = sine48
    r = lr.readout(E[:30], 48000)                       # 3 s
    h = bf.loudness_gate(48000, E[:30])
    print("997 Hz full scale: momentary %.4f (model), %.4f (host)" % (r.momentary, h.momentary))
    assert abs(r.momentary + 3.01) <= 0.01 and abs(h.momentary + 3.01) <= 0.01
    assert abs(r.momentary - h.momentary) <= 1e-9 and abs(r.short_term - h.short_term) <= 1e-9


def test_stereo_sine_at_minus_23(sine48):
    """EBU Tech 3341 case 1: the sine in two channels at -23 dBFS each reads -23.0 +- 0.1 LUFS integrated"""
    _, E1 = sine48
    g = 10.0 ** (-23.0 / 20.0)
    E = 2.0 * g * g * E1                                # two members, weight 1, the same signal scaled by g
    r, h = lr.readout(E, 48000), bf.loudness_gate(48000, E)
    print("stereo -23 dBFS: integrated %.4f (model), %.4f (host)" % (r.integrated, h.integrated))
    assert abs(r.integrated + 23.0) <= 0.1 and abs(h.integrated + 23.0) <= 0.1
    assert abs(r.integrated - h.integrated) <= 1e-9


def gating_programme(fs=8000):
    """two channels, a 997 Hz sine in both: 2 s at -40 dBFS, 2 s at -20 dBFS, 2 s of zeros -> v [frames][2]"""
    s = lr.sine(fs, 2.0)
    one = np.concatenate([s * 10.0 ** (-40 / 20.0), s * 10.0 ** (-20 / 20.0), np.zeros(2 * fs)])
    return np.stack([one, one], axis=1)


def test_gating():
    fs = 8000
    v = gating_programme(fs)
    E = lr.group_energy(v, fs)
    r, h = lr.readout(E, fs), bf.loudness_gate(fs, E)
    plain = lr.ungated(E, fs)
    print("gating: integrated %.3f (model), %.3f (host), ungated %.3f" % (r.integrated, h.integrated, plain))
    assert abs(r.integrated + 20.590) <= 2e-3 and abs(plain + 24.714) <= 2e-3      # the figures of the definition
    assert abs(h.integrated - r.integrated) <= 1e-9
    assert h.integrated > plain + 3.0
    assert (h.subblocks, h.first, h.wrapped) == (60, 0, False) == (r.subblocks, r.first, r.wrapped)
    for x, y in ((h.momentary, r.momentary), (h.short_term, r.short_term)):
        assert x == y or abs(x - y) <= 1e-9
    z = bf.loudness_gate(fs, np.zeros(60))
    assert z.momentary == z.short_term == z.integrated == -math.inf
    zm = lr.readout(np.zeros(60), fs)
    assert zm.momentary == zm.short_term == zm.integrated == -math.inf
    few = bf.loudness_gate(fs, E[20:23])                # three sub-blocks: nothing is defined yet
    assert few.momentary == few.short_term == few.integrated == -math.inf and few.subblocks == 3


def test_host_energy_matches_the_model():
    """both walk frame by frame in float64: they differ by FMA contraction at most"""
    fs = 8000
    rng = np.random.default_rng(3)
    v = rng.standard_normal(5 * fs + 123) * 0.2
    v[1000] = np.nan                                    # counts as 0
    v[1001] = np.inf
    got, want = bf.loudness_energy(fs, v), lr.channel_energy(v, fs)
    assert len(got) == len(want) == 50
    err = np.abs(got / want - 1.0).max()
    print("host energy against the model: worst relative error %.3g (bar 1e-12)" % err)
    assert err <= 1e-12
    assert len(bf.loudness_energy(fs, v[:799])) == 0 and len(bf.loudness_energy(fs, v[:800])) == 1
    assert np.array_equal(bf.loudness_energy(fs, np.zeros(1600)), np.zeros(2))
