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


# ------------------------------------------------------------------ networks

def _net_run(spec, nblk, actions, seed=9, amplitude=0.1):
    """the spec through the oracle's float64 engine and the model: -> (oracle, model) [frames][O]"""
    e = cases.build(bo.Engine, spec)
    blocks = cases.raw_blocks(seed, nblk, spec["L"], spec["n_in"], spec["infmt"], amplitude=amplitude)
    out = []
    for k, b in enumerate(blocks):
        for a in actions.get(k, ()):
            cases.act(e, a)
        st, raw = e.block(b)
        assert st == 0, k
        out.append(raw)
    got = xr.decode(np.concatenate(out), spec["outfmt"], spec["n_out"])
    x = xr.decode(np.concatenate(blocks), spec["infmt"], spec["n_in"])
    return got, xr.Network(spec).output(x, nblk, actions)


def _hold_blocks(got, want, L, tol=1e-11):
    """per block and output: relative RMS error, against the block's RMS or, for a block that is
    (nearly) silent, against 1e-3 of the output's RMS per block over the run"""
    nblk = len(want) // L
    for c in range(want.shape[1]):
        floor = 1e-3 * np.sqrt((want[:, c] ** 2).sum() / nblk)
        for k in range(nblk):
            s = slice(k * L, (k + 1) * L)
            err = np.sqrt(((got[s, c] - want[s, c]) ** 2).sum())
            assert err <= tol * max(np.sqrt((want[s, c] ** 2).sum()), floor), (k, c, err)


def test_model_matches_the_fade_cascade_network():
    """cases.fade_cascade_network's engine run (the oracle, float64) and its hand-written model, both
    held to the network model built from the same description"""
    got, hand, L, sw = cases.fade_cascade_network(bo.Engine, 8)
    L_, N, nblk, sw_, (ha, hb, hc, hd), x = cases.fade_cascade_parts()
    assert (L_, sw_, nblk * L) == (L, sw, len(got))
    spec = dict(L=L, N=N, n_out=2, coeffs=[(h, 1.0, 0) for h in (ha, hb, hc, hd)], filters=[
        dict(in_ch=[0], coeff=0, delayblocks=1),
        dict(in_ch=[1], coeff=1),
        dict(in_ch=[0], in_scale=[0.25], in_f=[0, 1], in_fscale=[0.5, -1.0], out_ch=[0], out_scale=[0.8],
             coeff=2, crossfade=True),
        dict(in_ch=[1], out_ch=[1, 0], out_scale=[1.0, -0.5], coeff=3, delayblocks=2)])
    want = xr.Network(spec).output(x, nblk, {sw: [("coeff", 2, 3)]})
    _hold_blocks(got, want, L)
    _hold_blocks(hand, want, L, 1e-13)


def _feature_spec(L, N, rs=8, infmt="S24_4LE", outfmt="FLOAT64_LE"):
    """the network of test_gpu_lengths.test_every_filter_feature_at_16384: a cascade with a mixed
    channel + filter input, a dirac clamped from delay 7, a multi-output filter, a scaled short set"""
    coeffs = [(_ir(210 + k, L * N, 2), 1.0, 0) for k in range(3)] + [(_ir(214, L, 2), 0.5, 1)]
    filters = [
        dict(in_ch=[0], coeff=0, out_ch=[2], crossfade=True),
        dict(in_ch=[1], coeff=1, delayblocks=1),
        dict(in_f=[0, 1], in_fscale=[1.0, -0.5], out_ch=[0], coeff=2, crossfade=True),
        dict(in_ch=[0, 1], in_scale=[0.5, 0.25], in_f=[1], out_ch=[1], coeff=3),
        dict(in_ch=[1], out_ch=[0, 1], out_scale=[0.25, -1.0], coeff=-1, delayblocks=7),
    ]
    return dict(L=L, N=N, rs=rs, n_in=2, n_out=3, infmt=infmt, outfmt=outfmt, coeffs=coeffs, filters=filters)


FEATURE_ACTIONS = {2: [("coeff", 0, 1)], 3: [("coeff", 2, -1), ("scale", 3, 0, 1, -0.75)],
                   4: [("coeff", 0, 0), ("coeff", 2, 2), ("fscale", 2, 1, 0.3)],
                   5: [("coeff", 2, 0), ("scale", 4, 1, 0, 2.0)],
                   7: [("fscale", 3, 0, -1.5), ("scale", 1, 0, 0, 0.5)]}


def test_model_matches_the_every_feature_network():
    """with the lengths test's switch sequence (hard and cross-faded, to and from a dirac) and, on
    top, in/out scale and fscale changes (slot by slot, the eval half of the block before)"""
    spec = _feature_spec(64, 3)
    got, want = _net_run(spec, 12, FEATURE_ACTIONS)
    _hold_blocks(got, want, 64)


def random_dag(rng, L, N, n_in, n_out, n_filters=6, n_coeffs=5):
    """a random cases.build network: every filter reads 0-2 channels and (after the first two) 0-2
    earlier filters, writes 0-2 outputs (at least one filter per output), a delay up to N + 1, a
    dirac or one of the sets (full, one tap into the last partition, short and scaled)"""
    lens = [N * L, (N - 1) * L + 1, L * N - L // 2, 2 * L, L]
    coeffs = [(rng.standard_normal(lens[k % 5]) / np.sqrt(lens[k % 5]) / 4, [1.0, 1.0, 0.5, -2.0, 1.0][k % 5],
               [0, 0, 0, 0, 1][k % 5]) for k in range(n_coeffs)]
    filters = []
    for f in range(n_filters):
        ins = sorted(rng.choice(n_in, int(rng.integers(0 if f >= 2 else 1, 3)), replace=False).tolist())
        fin = sorted(rng.choice(f, int(rng.integers(0, min(f, 2) + 1)), replace=False).tolist()) if f >= 2 else []
        if not ins and not fin:
            ins = [int(rng.integers(n_in))]
        outs = sorted(rng.choice(n_out, int(rng.integers(0, 3)), replace=False).tolist())
        filters.append(dict(in_ch=ins, in_scale=rng.uniform(-1, 1, len(ins)).round(3).tolist(), in_f=fin,
                            in_fscale=rng.uniform(-1, 1, len(fin)).round(3).tolist(), out_ch=outs,
                            out_scale=rng.uniform(-1.5, 1.5, len(outs)).round(3).tolist(),
                            coeff=int(rng.integers(-1, n_coeffs)), delayblocks=int(rng.integers(0, N + 2)),
                            crossfade=bool(rng.integers(2))))
    for o in range(n_out):
        if not any(o in fd["out_ch"] for fd in filters):
            fd = filters[int(rng.integers(n_filters))]
            fd["out_ch"].append(o)
            fd["out_scale"].append(1.0)
    return coeffs, filters


def random_actions(rng, filters, n_coeffs, t0, t1, n=6):
    """n run-time calls on random filters between blocks t0 and t1"""
    acts = {}
    for _ in range(n):
        t = int(rng.integers(t0, t1))
        f = int(rng.integers(len(filters)))
        fd = filters[f]
        kinds = ["coeff", "coeff"] + (["in"] if fd["in_ch"] else []) + (["out"] if fd["out_ch"] else []) + \
            (["fs"] if fd["in_f"] else [])
        k = kinds[int(rng.integers(len(kinds)))]
        v = round(float(rng.uniform(-1.5, 1.5)), 3)
        if k == "coeff":
            a = ("coeff", f, int(rng.integers(-1, n_coeffs)))
        elif k == "in":
            a = ("scale", f, 0, int(rng.integers(len(fd["in_ch"]))), v)
        elif k == "out":
            a = ("scale", f, 1, int(rng.integers(len(fd["out_ch"]))), v)
        else:
            a = ("fscale", f, int(rng.integers(len(fd["in_f"]))), v)
        acts.setdefault(t, []).append(a)
    return acts


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_model_matches_a_random_dag(seed):
    L_, N_, I, O = 32, 5, 3, 3
    rng = np.random.default_rng(seed)
    coeffs, filters = random_dag(rng, L_, N_, I, O)
    spec = dict(L=L_, N=N_, rs=8, n_in=I, n_out=O, infmt="FLOAT64_LE", outfmt="FLOAT64_LE", coeffs=coeffs,
                filters=filters)
    nblk = 3 * N_ + 2
    got, want = _net_run(spec, nblk, random_actions(rng, filters, len(coeffs), 1, nblk - 1, 8))
    _hold_blocks(got, want, L_)
