"""CPU: the channel stage of the float64 crossbar model (xbar_ref.Channels) held to the oracle's
float64 engine (bforacle.Engine), which implements all of it the reference's way: packed S24_LE
inputs, 0,1,0,1 maps on both sides beside a 1:1 channel, member delays in the short and the long
regime of the delay line, a muted member on each side, sub-sample filters on a raw input, a shared
input, a 1:1 output (in place) and a member of a shared output, unfiltered members beside them (the
sdf_length compensation), one run-time set_subdelay, and an HP-TPDF dithered output.

    float outputs   within 1e-12 relative RMS per block and channel
    S16_LE outputs  exact, except samples within 1e-6 LSB of a rounding threshold (1 count there);
                    one shared output clips: overflow records equal on every member (`largest`, a
                    double taken from the sample value itself, to 1e-12)"""
import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_ref as nr
import xbar_ref as xr


def oracle_run(spec, ch, actions, raw, nblk):
    e = cases.build_channels(bo.Engine, spec, ch)
    step = len(raw) // nblk
    outs = []
    for b in range(nblk):
        for a in actions.get(b, ()):
            cases.act(e, a)
        st, o = e.block(raw[b * step:(b + 1) * step])
        assert st == 0, b
        outs.append(o)
    return np.concatenate(outs), e


@pytest.mark.parametrize("L,half", [(64, 7), (256, 31)])
def test_float_outputs(L, half):
    N, nblk = 3, 9
    spec, ch, actions = cases.channel_stage(L, N, 8, "FLOAT64_LE", half)
    model = xr.Channels(spec, ch, cases.subdelay_taps(half, 8))
    raw = cases.packed_input(L, nblk * L, model.formats(0))
    y, _, _, status = model.run(raw, nblk, actions)
    got_raw, _ = oracle_run(spec, ch, actions, raw, nblk)
    got = nr.decode(got_raw, model.formats(1), nblk * L)
    assert status == [0] * nblk
    worst = 0.0
    for c in range(y.shape[1]):
        floor = 1e-3 * np.sqrt((y[:, c] ** 2).sum() / nblk)
        for b in range(nblk):
            s = slice(b * L, (b + 1) * L)
            err = np.sqrt(((got[s, c] - y[s, c]) ** 2).sum()) / max(np.sqrt((y[s, c] ** 2).sum()), floor, 1e-300)
            assert err <= 1e-12, (b, c, err)
            worst = max(worst, err)
    print("channel model vs oracle L=%d: worst rel rms %.3g" % (L, worst))


@pytest.mark.parametrize("L,half", [(64, 7), (256, 31)])
def test_integer_outputs_and_overflow_records(L, half):
    N, nblk = 3, 9
    spec, ch, actions = cases.channel_stage(L, N, 8, "S16_LE", half, dither=(2,), loud=6.0)
    model = xr.Channels(spec, ch, cases.subdelay_taps(half, 8))
    raw = cases.packed_input(L + 1, nblk * L, model.formats(0))
    y, want_raw, ofs, status = model.run(raw, nblk, actions)
    got_raw, e = oracle_run(spec, ch, actions, raw, nblk)
    assert status == [0] * nblk
    got, want = nr.ints(got_raw, model.formats(1), nblk * L), nr.ints(want_raw, model.formats(1), nblk * L)
    u = y * 32768.0 + 0.5
    near = np.abs(u - np.round(u)) < 1e-6
    diff = np.abs(got - want)
    assert diff[:, :2][~near[:, :2]].max() == 0 and diff[:, :2].max() <= 1
    assert diff[:, 2].max() == 0                        # the dithered 1:1 output: the same table walk
    assert ofs[1].n_overflows > 0 and ofs[0].n_overflows == 0
    for v in range(5):
        g, w = e.overflow(v), ofs[v]
        assert (g.n_overflows, g.intlargest, g.max) == (w.n_overflows, w.intlargest, w.max), v
        assert g.largest == pytest.approx(w.largest, rel=1e-12), v
    assert ofs[1].astuple() == ofs[3].astuple()
