"""The float64 crossbar model (tests/xbar_ref.py) against the oracle's float64 engine, at a small
length: the model has to be right before it judges the GPU's long-window plan
(tests/test_gpu_long_window_ref.py).  Covered: block delays (clamped ones too), short sets, hard and
cross-faded switches, in-place partition rewrites (a switch to the rewritten set in the oracle), a
run-time delay change, scale changes, an N:1 input map with a muted and a sample-delayed virtual
input, and S16 clipping with its overflow records."""
import numpy as np
import pytest

import bforacle as bo
import cases
import xbar_ref as xr

L, N = 256, 6


def _ir(seed, taps, n_in=3):
    return cases.make_ir(np.random.default_rng(seed), taps, n_in)


def _run(e, blocks, actions):
    out, sts = [], []
    for k, b in enumerate(blocks):
        for a in actions.get(k, ()):
            a()
        st, raw = e.block(b)
        sts.append(st)
        out.append(raw)
    return sts, out


@pytest.mark.parametrize("fade", [False, True])
def test_model_matches_the_oracle_through_switches_rewrites_and_delays(fade):
    I, O = 3, 2
    nblk = 4 * N + 3
    lengths = {(0, 0): N * L, (0, 1): 3 * L + 17, (0, 2): N * L, (1, 0): N * L - 5, (1, 1): 2 * L, (1, 2): N * L}
    delays = {(0, 0): 0, (0, 1): 2, (0, 2): N + 1, (1, 0): N - 1, (1, 1): 1, (1, 2): N - 2}
    irs = {k: _ir(100 + 7 * k[0] + k[1], n) for k, n in lengths.items()}
    alt = _ir(200, N * L)
    part = _ir(201, L)
    e = bo.Engine(L, N, 8, I, O)
    e.set_interleaved(0, "S24_4LE")
    e.set_interleaved(1, "FLOAT64_LE")
    model, fidx = [], {}
    for (o, i), h in irs.items():
        c = e.add_coeff(h)
        fidx[(o, i)] = e.add_filter(in_ch=[i], out_ch=[o], coeff=c, delayblocks=delays[(o, i)], crossfade=fade,
                                    in_scale=[0.75 if i == 1 else 1.0], out_scale=[-1.25 if o == 1 else 1.0])
        model.append(xr.Filter(i, o, h, delays[(o, i)], 0.75 if i == 1 else 1.0, -1.25 if o == 1 else 1.0))
    c_alt = e.add_coeff(alt)
    rewritten = irs[(0, 0)].copy()
    rewritten[4 * L:5 * L] = part                       # partition 4 of set (0, 0) rewritten in place
    c_rw = e.add_coeff(rewritten)
    sw, rw, dl, sc = N + 1, N + 4, 2 * N + 2, 3 * N
    f00, f01, f10, f11 = fidx[(0, 0)], fidx[(0, 1)], fidx[(1, 0)], fidx[(1, 1)]
    actions = {sw: [lambda: e.set_coeff(f10, c_alt)],
               rw: [lambda: e.set_coeff(f00, c_rw)],
               dl: [lambda: e.set_delayblocks(f01, 0), lambda: e.set_delayblocks(f11, N - 3)],
               sc: [lambda: e.set_scale(f11, 0, 0, -0.5), lambda: e.set_scale(f10, 1, 0, 2.0)]}
    model[f10].change(sw, fade=fade, taps=alt)
    model[f00].change(rw, fade=fade, taps=rewritten)
    model[f01].change(dl, delay=0)
    model[f11].change(dl, delay=N - 3)
    model[f11].change(sc, in_scale=-0.5)
    model[f10].change(sc, out_scale=2.0)
    blocks = cases.raw_blocks(5, nblk, L, I, "S24_4LE")
    sts, out = _run(e, blocks, actions)
    assert sts == [0] * nblk
    got = np.concatenate([np.frombuffer(r.tobytes(), np.float64).reshape(L, O) for r in out])
    x = xr.decode(np.concatenate(blocks), "S24_4LE", I)
    want = xr.output(x, model, L, N, O, nblk)
    for k in range(nblk):
        s = slice(k * L, (k + 1) * L)
        assert cases.rel_rms(got[s], want[s]) <= 1e-11, k
    # the model is not blind: without the rewrite it differs from block rw on
    model[f00].segs.pop()
    off = xr.output(x, model, L, N, O, nblk)
    assert cases.rel_rms(off[rw * L:(rw + 1) * L], want[rw * L:(rw + 1) * L]) > 1e-3


def test_model_matches_the_oracle_on_an_input_map_with_mute_and_sample_delay():
    """virtual inputs 0 and 1 read physical channel 0; virtual 1 is delayed by 37 samples, virtual 0
    is muted from block `m` on; virtual 2 reads physical channel 1"""
    O, n_phys = 2, 2
    v2p = [0, 0, 1]
    nblk, m = 3 * N, N + 2
    e = bo.Engine(L, N, 8, len(v2p), O)
    e.map_channels(0, v2p)
    e.set_interleaved_phys(0, "FLOAT_LE", n_phys)
    e.set_interleaved(1, "FLOAT64_LE")
    e.set_maxdelay(0, 1, 100)                        # a delay that may change at run time
    e.set_delay(0, 1, 37)
    model = []
    for o in range(O):
        for v in range(len(v2p)):
            h = _ir(300 + o * 3 + v, N * L)
            e.add_filter(in_ch=[v], out_ch=[o], coeff=e.add_coeff(h))
            model.append(xr.Filter(v, o, h))
    blocks = cases.raw_blocks(6, nblk, L, n_phys, "FLOAT_LE")
    sts, out = _run(e, blocks, {m: [lambda: e.set_mute(0, 0, 1)]})
    assert sts == [0] * nblk
    got = np.concatenate([np.frombuffer(r.tobytes(), np.float64).reshape(L, O) for r in out])
    x = xr.virtual_inputs(xr.decode(np.concatenate(blocks), "FLOAT_LE", n_phys), v2p, delay={1: 37},
                          mute_from={0: m}, L=L)
    want = xr.output(x, model, L, N, O, nblk)
    for k in range(nblk):
        s = slice(k * L, (k + 1) * L)
        assert cases.rel_rms(got[s], want[s]) <= 1e-11, k


@pytest.mark.parametrize("fmt", ["S16_LE", "S24_LE", "S32_LE"])
def test_model_requantises_and_counts_overflows_like_the_oracle(fmt):
    I, O = 2, 3
    nblk = 2 * N + 1
    e = bo.Engine(L, N, 8, I, O)
    e.set_interleaved(0, "S16_LE")
    e.set_interleaved(1, fmt)
    model = []
    for o in range(O):
        for i in range(I):
            h = _ir(400 + o * I + i, N * L, 1) * (40.0 if o == 1 else 0.5)     # output 1 clips
            e.add_filter(in_ch=[i], out_ch=[o], coeff=e.add_coeff(h))
            model.append(xr.Filter(i, o, h))
    blocks = cases.raw_blocks(7, nblk, L, I, "S16_LE", amplitude=0.4)
    sts, out = _run(e, blocks, {})
    assert sts == [0] * nblk
    x = xr.decode(np.concatenate(blocks), "S16_LE", I)
    y = xr.output(x, model, L, N, O, nblk)
    want, ofs, st = xr.encode(y, fmt, L)
    assert st == [0] * nblk
    got = xr.decode(np.concatenate(out), fmt, O) * float(1 << (8 * xr.FORMATS[fmt][1] - 1))
    assert np.abs(got - want).max() <= (0 if fmt == "S16_LE" else 1)
    assert ofs[1].n_overflows > 0 and ofs[0].n_overflows == 0
    for c in range(O):
        g = e.overflow(c)
        assert g.n_overflows == ofs[c].n_overflows and g.max == ofs[c].max, c
        assert abs(g.intlargest - ofs[c].intlargest) <= (0 if fmt == "S16_LE" else 1), c
        assert g.largest == pytest.approx(ofs[c].largest, rel=1e-9, abs=1e-9), c
