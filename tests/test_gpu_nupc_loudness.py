"""GPU: the BS.1770 loudness meter on the non-uniform convolver's outputs (include/bfhip_nupc.h) against the
float64 model of tests/loudness_ref.py (held to the standard in tests/test_loudness_model.py).

The model's input is always the bytes the convolver itself returned (loudness_ref.decode), so only the meter's
error is measured.  Unless a case says otherwise: 2 inputs, fs = 8000 (S = 800 frames), every output fed from
one input through a short flat-noise filter, input noise at 0.05 with x8 bursts plus a 997 Hz sine: zero mean,
energy above 100 Hz, so the high-pass cancels nothing large and a relative bar is fair.

Bars (the device and the model do the same float64 arithmetic in another order): 1e-9 relative on every E_g[j],
1e-8 LU on every finite read-out, exactly 0 where the model's E is exactly 0.  A sub-block sum of S = 800
positive terms moves by at most S 2^-53 = 1e-13 under reordering, the sections' rounding noise is about
2^-53 / (1 - r) with r = 0.97 at fs 8000, and the chunked scan adds a few such terms per chunk edge.  Each test
prints its worst error as a fraction of the bar.

Measured worst on the MI355X: E within 1.4e-14 relative (1.4e-5 of the bar) in every case but one, read-outs within
7.1e-15 LU (7.1e-7 of the bar).  The one: the gating programme's sub-block 55, deep in the silence, where the
filters' decaying tail leaves E near 5e-314, a subnormal number with 33 or 34 significant bits left: the device and
the model differ there by 7.5e-11 relative (0.075 of the bar), one unit in the last place of such a number -- the
format's resolution, not the meter's.  Sub-blocks 56 .. 59 are exactly 0 on both sides."""
import ctypes as C
import math

import numpy as np
import pytest

import loudness_ref as lr
from test_loudness_model import gating_programme

pytestmark = pytest.mark.gpu
FS, S = 8000, 800
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
IN, OUT = 0, 1
ESTATE, EINVAL = -5, -1
E_BAR, LU_BAR = 1e-9, 1e-8
SMALL = ([64, 128], [2, 2])


def _input(rs, frames, n_in=2, seed=0):
    rng = np.random.default_rng(100 + seed)
    x = rng.standard_normal((frames, n_in)) * 0.05
    for at in range(300, frames - 200, 2900):
        x[at:at + 150] *= 8.0
    x += 0.1 * lr.sine(FS, frames / FS)[:frames, None] * np.array([1.0, -0.7])[:n_in]
    return np.ascontiguousarray(x.astype(np.float32 if rs == 4 else np.float64))


def _make(hip, rs, sched, n_out, groups=(), outfmt=None, fmts=None, buf_bytes=None, history=36000, meter=True, setup=None,
          gain=1.0, one_tap=False):
    """groups: [(channels, weights or None)]; fmts / buf_bytes: a declared output buffer (period_layout) -> (nu, fmts)"""
    dt = np.float32 if rs == 4 else np.float64
    nu = hip.Nupc(sched[0], sched[1], rs, 2, n_out)
    nu.set_interleaved(IN, FF[rs])
    if fmts is None:
        fmts = hip.interleaved_formats(outfmt or FF[rs], n_out)
    for c, f in enumerate(fmts):
        nu.set_format(OUT, c, f)
    if buf_bytes:
        nu.set_buffer_bytes(OUT, buf_bytes)
    rng = np.random.default_rng(7)
    for o in range(n_out):
        h = np.ones(1) if one_tap else rng.standard_normal(24) / np.sqrt(24) * (1.0 + 0.2 * o)
        nu.add_filter(o % 2, o, (h * gain).astype(dt))
    if setup:
        setup(nu)
    if meter:
        nu.enable_loudness(FS, history)
        for k, (chs, w) in enumerate(groups):
            assert nu.add_loudness_group(chs, w) == k
    nu.finalize()
    return nu, fmts


def _run(nu, x, periods, before=None):
    L0, out, sts = nu.L0, [], []
    for p in range(periods):
        if before:
            before(p)
        st, y = nu.block(x[p * L0:(p + 1) * L0])
        sts.append(st)
        out.append(y)
    return np.concatenate(out), sts


def _close(tag, got, want):
    """every E against the model's: 1e-9 relative, exactly 0 where the model's is -> worst error / bar"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), tag
    rel = np.abs(got[~zero] / want[~zero] - 1.0) if (~zero).any() else np.zeros(1)
    print("%s: %d sub-blocks, worst relative error %.3g = %.3g of the bar" % (tag, len(want), rel.max(), rel.max() / E_BAR))
    assert rel.max() <= E_BAR, (tag, int(rel.argmax()), rel.max())
    return rel.max() / E_BAR


def _same_readout(tag, got, want):
    worst = 0.0
    for name in ("momentary", "short_term", "integrated"):
        a, b = getattr(got, name), getattr(want, name)
        if math.isinf(b) or math.isinf(a):
            assert a == b, (tag, name, a, b)
        else:
            worst = max(worst, abs(a - b))
            assert abs(a - b) <= LU_BAR, (tag, name, a, b)
    assert (got.subblocks, got.first, bool(got.wrapped)) == (want.subblocks, want.first, bool(want.wrapped)), (tag, got, want)
    print("%s: read-outs %.4f / %.4f / %.4f LUFS, worst error %.3g LU = %.3g of the bar"
          % (tag, got.momentary, got.short_term, got.integrated, worst, worst / LU_BAR))


def _hold(tag, nu, raw, fmts, groups, history=None, resets=None):
    """every group of the metered convolver against the model on the bytes it returned"""
    v = lr.decode(raw, fmts, nu.L0, nu.out_bytes)
    n_sub = len(v) // S
    out = []
    for g, (chs, w) in enumerate(groups):
        want = lr.group_energy(v[:, list(chs)], FS, w)
        assert len(want) == n_sub
        oldest = max(n_sub - history, 0) if history else 0
        got = nu.loudness_energy(g, oldest, n_sub - oldest)
        _close("%s group %d" % (tag, g), got, want[oldest:])
        r = nu.loudness(g)
        reset = (resets or {}).get(g, 0)
        dev_e = np.concatenate([np.zeros(oldest), got])               # (cells in front of `oldest` are never read)
        _same_readout("%s group %d on the device's E" % (tag, g), r, lr.readout(dev_e, FS, reset, history))
        _same_readout("%s group %d on the model's E" % (tag, g), r, lr.readout(want, FS, reset, history))
        out.append((got, r))
    return out


# ---------------------------------------------------------------- A. energies

@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("sched,seconds", [(([64, 128], [2, 2]), 3.5),       # a boundary in mid-period: 12.5 periods per sub-block
                                           (([16, 32], [2, 2]), 1.0),        # sub-blocks spanning many periods
                                           (([2048], [2]), 2.0)])            # several sub-blocks inside one period; the chunked scan
def test_energies(hip, rs, sched, seconds):
    L0 = sched[0][0]
    periods = -(-int(seconds * FS) // L0)
    groups = [((0, 1), None)]
    nu, fmts = _make(hip, rs, sched, 2, groups)
    raw, sts = _run(nu, _input(rs, periods * L0), periods)
    assert not any(sts)
    (E, r), = _hold("A rs %d L0 %d" % (rs, L0), nu, raw, fmts, groups)
    assert len(E) == periods * L0 // S and E.min() > 0
    assert math.isfinite(r.momentary) and math.isfinite(r.integrated) and math.isfinite(r.short_term) == (seconds >= 3.0)
    nu.close()


def test_energies_long_period(hip):
    """L0 = 16384: two tiles of the chunked scan per period, twenty sub-blocks inside one period"""
    sched, rs = ([16384], [1]), 8
    groups = [((0, 1), None)]
    nu, fmts = _make(hip, rs, sched, 2, groups)
    raw, sts = _run(nu, _input(rs, 2 * 16384), 2)
    assert not any(sts)
    (E, _), = _hold("A L0 16384", nu, raw, fmts, groups)
    assert len(E) == 40
    nu.close()


# ---------------------------------------------------------------- B. what leaves is what is metered

def test_dithered_s16(hip):
    groups = [((0, 1), None)]
    nu, fmts = _make(hip, 8, SMALL, 2, groups, outfmt="S16_LE", setup=lambda nu: nu.enable_dither([0, 1], FS))
    raw, _ = _run(nu, _input(8, 125 * 64), 125)
    _hold("B dither S16", nu, raw, fmts, groups)
    nu.close()


def test_delay_and_mute(hip):
    groups = [((0, 1, 2), None)]

    def setup(nu):
        nu.set_maxdelay(OUT, 0, 128)
        nu.set_delay(OUT, 0, 37)

    nu, fmts = _make(hip, 4, SMALL, 3, groups, outfmt="S32_LE", setup=setup)

    def before(p):
        if p == 60:
            nu.set_mute(OUT, 1, True)

    raw, _ = _run(nu, _input(4, 125 * 64), 125, before)
    v = lr.decode(raw, fmts, 64, nu.out_bytes)
    assert not v[:37, 0].any() and v[37:200, 0].any() and v[:60 * 64, 1].any() and not v[60 * 64:, 1].any()
    _hold("B delay, mute", nu, raw, fmts, groups)
    nu.close()


def test_limited_true_peak(hip):
    groups = [((0, 1), None)]

    def setup(nu):
        nu.enable_limiter(64, 500.0)
        nu.set_limiter_detector(hip.LIMIT_TRUE_PEAK)
        nu.add_limiter_group([0, 1], 0.25)

    nu, fmts = _make(hip, 8, SMALL, 2, groups, setup=setup, gain=4.0)
    raw, _ = _run(nu, _input(8, 125 * 64), 125)
    assert nu.limiter_reduction(0) < 0.7                                 # it did limit
    _hold("B limiter", nu, raw, fmts, groups)
    nu.close()


def test_planar_layout(hip):
    groups = [((1, 0), (1.0, 0.5))]
    fmts, n_bytes = hip.period_layout(64, [("FLOAT_LE", 2, [0, 1], False)])
    nu, fmts = _make(hip, 4, SMALL, 2, groups, fmts=fmts, buf_bytes=n_bytes)
    raw, _ = _run(nu, _input(4, 125 * 64), 125)
    _hold("B planar", nu, raw, fmts, groups)
    nu.close()


def test_second_device_of_packed_24_bit(hip):
    """an interleaved float device and a second, non-interleaved one of S24_LE (three bytes a sample)"""
    groups = [((0, 1, 2, 3), None), ((2, 3), None)]
    fmts, n_bytes = hip.period_layout(64, [("FLOAT64_LE", 2, [0, 1], True), ("S24_LE", 2, [0, 1], False)])
    nu, fmts = _make(hip, 8, SMALL, 4, groups, fmts=fmts, buf_bytes=n_bytes)
    raw, _ = _run(nu, _input(8, 125 * 64), 125)
    _hold("B two devices", nu, raw, fmts, groups)
    nu.close()


# ---------------------------------------------------------------- C. groups

def test_groups(hip):
    """five members with the surround weights; channel 1 in two groups; a weight of 0 contributes exactly nothing:
    the bits of the group without that member"""
    groups = [((0, 1, 2, 4, 5), (1.0, 1.0, 1.0, 1.41, 1.41)), ((1, 3), None), ((0, 2), (0.0, 1.0)), ((2,), None)]
    nu, fmts = _make(hip, 8, SMALL, 6, groups)
    raw, _ = _run(nu, _input(8, 125 * 64), 125)
    res = _hold("C", nu, raw, fmts, groups)
    assert np.array_equal(res[2][0], res[3][0]) and res[2][0].min() > 0
    assert res[2][1] == res[3][1]
    nu.close()


# ---------------------------------------------------------------- D. gating on the device

def test_gating_and_reset(hip):
    """the -40 / -20 / silence programme of the model test through one-tap filters, 750 periods of 64 frames"""
    groups = [((0, 1), None), ((0, 1), None)]
    nu, fmts = _make(hip, 8, SMALL, 2, groups, one_tap=True)
    x = gating_programme(FS)

    def before(p):
        if p == 375:                                                     # 3 s: frame 24 000 is the first of sub-block 30
            nu.reset_loudness(1)

    raw, _ = _run(nu, x, 750, before)
    (E, r0), (_, r1) = _hold("D", nu, raw, fmts, groups, resets={1: 30})
    plain = lr.ungated(E, FS)
    print("D: integrated %.3f, ungated %.3f, after the reset %.3f" % (r0.integrated, plain, r1.integrated))
    assert r0.integrated > plain + 3.0 and abs(r0.integrated + 20.590) < 2e-3
    assert (r0.first, r1.first) == (0, 30) and not r0.wrapped and not r1.wrapped
    assert abs(r1.integrated - lr.readout(E[30:], FS).integrated) <= LU_BAR and r1.integrated != r0.integrated
    assert r0.momentary == -math.inf and r1.momentary == -math.inf      # the last 400 ms are silence: E is exactly 0
    nu.reset_loudness(0)                                                 # nothing complete behind it yet
    assert nu.loudness(0).integrated == -math.inf and nu.loudness(0).first == 60
    nu.close()


# ---------------------------------------------------------------- E. ring wrap

def test_ring_wrap(hip):
    groups = [((0, 1), None)]
    nu, fmts = _make(hip, 8, SMALL, 2, groups, history=30)
    raw, _ = _run(nu, _input(8, 563 * 64), 563)                          # 36 032 frames: 45 sub-blocks
    (E, r), = _hold("E", nu, raw, fmts, groups, history=30)
    assert r.wrapped and r.first == 15 and r.subblocks == 45 and len(E) == 30
    L = hip.lib()
    buf = np.full(2, -1.0)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.bfhip_nupc_get_loudness_energy(nu.h, 0, 14, 1, p) == EINVAL and b"left" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_get_loudness_energy(nu.h, 0, 45, 1, p) == EINVAL and b"complete" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_get_loudness_energy(nu.h, 0, 44, 2, p) == EINVAL and np.all(buf == -1.0)
    assert L.bfhip_nupc_get_loudness_energy(nu.h, 0, 43, 2, p) == 0 and np.array_equal(buf, E[-2:])
    nu.close()


# ---------------------------------------------------------------- F. the meter only reads

@pytest.mark.parametrize("rs,outfmt", [(4, None), (8, "S24_4LE")])
def test_the_meter_only_reads(hip, rs, outfmt):
    groups = [((0, 1), None), ((1,), (1.41,))]
    x = _input(rs, 100 * 64)
    runs = []
    for meter in (False, True, True):
        nu, _ = _make(hip, rs, SMALL, 2, groups, outfmt=outfmt, meter=meter, gain=12.0)
        raw, sts = _run(nu, x, 100)
        E = [nu.loudness_energy(g, 0, 8) for g in range(2)] if meter else None
        runs.append((raw, sts, E, [nu.overflow(c).astuple() for c in range(2)]))
        nu.close()
    assert runs[0][0].any() and np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][3] == runs[1][3]
    assert np.array_equal(runs[1][0], runs[2][0])
    for g in range(2):
        assert runs[1][2][g].tobytes() == runs[2][2][g].tobytes() and runs[1][2][g].min() > 0


# ---------------------------------------------------------------- G. misuse

def _code(call):
    import brutefir_amd as bf
    with pytest.raises(bf.BfhipError) as e:
        call()
    return int(str(e.value).split("error ")[1].split(":")[0])


def test_misuse(hip):
    L = hip.lib()
    err = lambda: L.bfhip_nupc_last_error().decode()
    nu = hip.Nupc([64], [2], 4, 2, 18)
    for o in range(18):
        nu.add_filter(0, o, np.ones(4, np.float32))
    assert _code(lambda: nu.add_loudness_group([0], None)) == ESTATE            # a group before enable
    for rate, hist in [(8001, 36000), (7990, 36000), (768010, 36000), (0, 36000), (48000, 29), (48000, (1 << 22) + 1)]:
        assert _code(lambda: nu.enable_loudness(rate, hist)) == EINVAL, (rate, hist)
    assert "30" in err()
    nu.enable_loudness(48000, 30)
    assert _code(lambda: nu.enable_loudness(48000, 30)) == ESTATE               # twice
    assert nu.add_loudness_group([0, 1], None) == 0
    assert _code(lambda: nu.add_loudness_group([18], None)) == EINVAL and "18" in err()
    assert _code(lambda: nu.add_loudness_group([-1], None)) == EINVAL
    assert _code(lambda: nu.add_loudness_group([2, 3, 2], None)) == EINVAL and "channel 2" in err()
    assert _code(lambda: nu.add_loudness_group([4, 5], [1.0, -0.5])) == EINVAL and "channel 5" in err()
    assert _code(lambda: nu.add_loudness_group([4, 5], [float("nan"), 1.0])) == EINVAL and "channel 4" in err()
    assert _code(lambda: nu.add_loudness_group([4, 5], [1.0, float("inf")])) == EINVAL
    assert _code(lambda: nu.add_loudness_group([], None)) == EINVAL and "16" in err()
    assert _code(lambda: nu.add_loudness_group(list(range(17)), None)) == EINVAL and "16" in err()
    assert nu.add_loudness_group(list(range(16)), None) == 1                    # nothing changed after the errors
    for k in range(2, 32):
        assert nu.add_loudness_group([0, 1], [1.0, 0.0]) == k                   # the same channels again: legal
    assert _code(lambda: nu.add_loudness_group([0], None)) == EINVAL and "32" in err()      # a 33rd group
    assert _code(lambda: nu.loudness(0)) == ESTATE                              # before finalize
    nu.finalize()
    assert _code(lambda: nu.enable_loudness(48000, 30)) == ESTATE               # after finalize
    assert _code(lambda: nu.add_loudness_group([4], None)) == ESTATE
    assert _code(lambda: nu.loudness(32)) == EINVAL and _code(lambda: nu.loudness(-1)) == EINVAL
    assert _code(lambda: nu.reset_loudness(32)) == EINVAL
    assert _code(lambda: nu.loudness_energy(0, 0, 1)) == EINVAL                 # nothing complete yet
    s = hip.LoudnessStruct(-3.0, 0, 0, 7, 0, 0)
    assert L.bfhip_nupc_get_loudness(nu.h, 0, None) == EINVAL
    assert L.bfhip_nupc_get_loudness(nu.h, 32, C.byref(s)) == EINVAL and (s.momentary, s.subblocks) == (-3.0, 7)
    r = nu.loudness(0)
    assert (r.momentary, r.short_term, r.integrated, r.subblocks, r.first, r.wrapped) == (-math.inf,) * 3 + (0, 0, False)
    st, y = nu.block(np.full((64, 2), 0.25, np.float32))
    assert st == 0 and y.any() and nu.loudness(31).subblocks == 0 and len(nu.loudness_energy(1, 0, 0)) == 0
    nu.close()
    plain = hip.Nupc([64], [2], 4, 1, 1)
    plain.add_filter(0, 0, np.ones(8, np.float32))
    assert _code(lambda: plain.loudness(0)) == ESTATE and _code(lambda: plain.reset_loudness(0)) == ESTATE
    plain.finalize()
    assert _code(lambda: plain.enable_loudness(48000, 36000)) == ESTATE
    assert _code(lambda: plain.add_loudness_group([0], None)) == ESTATE
    assert _code(lambda: plain.loudness(0)) == ESTATE
    assert _code(lambda: plain.loudness_energy(0, 0, 1)) == ESTATE
    assert _code(lambda: plain.reset_loudness(0)) == ESTATE
    assert plain.block(np.ones((64, 1), np.float32))[0] == 0
    plain.close()
