"""CPU: the float64 reference model of the non-uniform convolver (tests/nupc_ref.py) against the
oracle's uniform engine (oracle/bforacle.py, the reference's filter_process restated) in float64.
The GPU tests of the convolver (test_gpu_nupc_shapes.py) measure the library against this model,
so the model itself is held to the yardstick here: decoded inputs, scales, the convolution, the
one-block cross-fade, requantisation, dither and overflow counters.  Reals within 1e-12 relative
RMS, integer samples within 1 LSB (rounding ties), overflow counters equal."""
import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_ref as nr


def _oracle(L, N, n_in, n_out, fin, fout, filters, coeffs2=None, dither=(), rate=44100):
    oe = bo.Engine(L, N, 8, n_in, n_out)
    for io, fm in ((0, fin), (1, fout)):
        for c, f in enumerate(fm):
            oe.set_format(io, c, f)
    oe.out_bytes = L * nr.frame_bytes(fout)
    if dither:
        assert oe.enable_dither(list(dither), rate)
    for k, (i, o, h, si, so) in enumerate(filters):
        c = oe.add_coeff(h)
        if coeffs2 is not None:
            oe.add_coeff(coeffs2[k])
        oe.add_filter(in_ch=[i], out_ch=[o], coeff=c, in_scale=[si], out_scale=[so],
                      crossfade=coeffs2 is not None)
    return oe


def _raw_input(rng, fin, n, amp):
    x = np.zeros((n, len(fin)))
    for c, f in enumerate(fin):
        v = rng.standard_normal(n) * amp
        x[:, c] = v if f.isfloat else np.round(v / f.scale)
    return nr.pack(x, fin)


def _filters(rng, n_in, n_out, taps, pairs):
    out = []
    for i, o in pairs:
        h = cases.make_ir(rng, taps, n_in)
        out.append((i, o, h, float(rng.choice([1.0, 0.5, -1.0])), float(rng.choice([1.0, -0.25, 2.0]))))
    return out


def _run(oe, raw, L, fb_in, fb_out, n):
    got = []
    for b in range(n // L):
        st, r = oe.block(raw[b * L * fb_in:(b + 1) * L * fb_in])
        assert st == 0
        got.append(r)
    return np.concatenate(got)


@pytest.mark.parametrize("fin_names,fout_names,gap", [
    (["S16_LE", "S16_BE"], ["FLOAT64_LE", "FLOAT64_BE", "FLOAT64_LE"], 0),
    (["S24_4LE", "S32_BE", "FLOAT_LE"], ["FLOAT_BE", "S32_LE"], 1),
    (["FLOAT64_BE"], ["FLOAT64_LE"] * 2, 3),
])
def test_model_reals_equal_the_uniform_engine(fin_names, fout_names, gap):
    rng = np.random.default_rng(len(fin_names) * 10 + gap)
    L, N, n = 64, 4, 64 * 12
    fin = nr.layout(fin_names, gap=gap, order=list(range(len(fin_names)))[::-1])
    fout = nr.layout(fout_names, gap=gap)
    fl = [c for c, f in enumerate(fout) if f.isfloat]
    pairs = [(i, o) for o in range(len(fout)) for i in range(len(fin)) if (i + o) % 3 != 2]
    pairs.append(pairs[0])                                     # two filters on one pair
    filters = _filters(rng, len(fin), len(fout), L * N - 37, pairs)
    raw = _raw_input(rng, fin, n, 0.2)
    oe = _oracle(L, N, len(fin), len(fout), fin, fout, filters)
    got = nr.decode(_run(oe, raw, L, nr.frame_bytes(fin), nr.frame_bytes(fout), n), fout, n)
    y = nr.convolve(nr.decode(raw, fin, n), filters, len(fout))
    assert np.abs(y).max() > 0.01
    for c in fl:
        tol = 1e-12 if fout[c].bytes == 8 else 1e-7            # FLOAT_*: stored as float32
        assert cases.rel_rms(got[:, c], y[:, c]) <= tol, c
    # the model's float encoding is the float64 result, stored at the format's width
    want = nr.decode(nr.encode(y, fout, L)[0], fout, n)
    for c in fl:
        assert cases.rel_rms(got[:, c], want[:, c]) <= (1e-12 if fout[c].bytes == 8 else 1e-7), c


@pytest.mark.parametrize("outs", [["S16_LE", "S16_BE"], ["S24_LE", "S24_BE"], ["S8", "S8", "S8"],
                                  ["S32_LE", "S24_4BE", "S24_4LE"]])
def test_model_integers_and_overflows_equal_the_uniform_engine(outs):
    """loud enough that every integer output clips now and then; the clipped samples lie far from
    full scale, so both sides count the same ones"""
    rng = np.random.default_rng(len(outs) + sum(map(len, outs)))
    L, N, n = 32, 3, 32 * 20
    fin = nr.layout(["FLOAT64_LE"] * 2)
    fout = nr.layout(outs, gap=1, order=list(range(len(outs)))[::-1])
    filters = _filters(rng, 2, len(outs), L * N, [(i, o) for o in range(len(outs)) for i in range(2)])
    x = rng.standard_normal((n, 2)) * 20.0
    raw = nr.pack(x, fin)
    oe = _oracle(L, N, 2, len(outs), fin, fout, filters)
    got_raw = _run(oe, raw, L, nr.frame_bytes(fin), nr.frame_bytes(fout), n)
    y = nr.convolve(nr.decode(raw, fin, n), filters, len(outs))
    want_raw, of, st = nr.encode(y, fout, L)
    assert st == [0] * (n // L)
    got, want = nr.ints(got_raw, fout, n), nr.ints(want_raw, fout, n)
    assert np.abs(got - want).max() <= 1
    for c in range(len(outs)):
        o = oe.overflow(c)
        assert o.n_overflows == of[c].n_overflows > 0, c
        assert abs(o.intlargest - of[c].intlargest) <= 1 and o.max == of[c].max, c
        assert o.largest == pytest.approx(of[c].largest, rel=1e-9)


def test_model_dither_equals_the_uniform_engine():
    """HP-TPDF dither on one of three S16 outputs, slot 0: the model's period-by-period cbuf2raw
    walks the same table as the engine's"""
    rng = np.random.default_rng(5)
    L, N, n = 64, 2, 64 * 30
    fin = nr.layout(["FLOAT64_LE"] * 2)
    fout = nr.layout(["S16_LE"] * 3)
    filters = _filters(rng, 2, 3, L * N, [(0, 0), (1, 1), (0, 2), (1, 2)])
    raw = nr.pack(rng.standard_normal((n, 2)) * 0.2, fin)
    oe = _oracle(L, N, 2, 3, fin, fout, filters, dither=[1], rate=300)
    got = nr.ints(_run(oe, raw, L, 16, 6, n), fout, n)
    y = nr.convolve(nr.decode(raw, fin, n), filters, 3)
    want = nr.ints(nr.encode(y, fout, L, dither=[1], rate=300)[0], fout, n)
    d = np.abs(got - want)
    assert d.max() <= 1 and (d > 0).sum() <= 4, (d.max(), (d > 0).sum())
    # the dithered channel really is dithered: plain rounding differs from it
    plain = nr.ints(nr.encode(y, fout, L)[0], fout, n)
    assert (plain[:, 1] != want[:, 1]).sum() > n // 4
    assert np.array_equal(plain[:, [0, 2]], want[:, [0, 2]])


def test_model_crossfade_equals_the_uniform_engine():
    """the reference's one-block cross-fade (set_coeff at block b of a crossfade filter) is the
    model's blend at t_sw = b * L with F = L"""
    rng = np.random.default_rng(6)
    L, N, n, sw = 64, 3, 64 * 14, 6
    fin = nr.layout(["FLOAT64_LE"] * 2)
    fout = nr.layout(["FLOAT64_LE"] * 2)
    filters = _filters(rng, 2, 2, L * N, [(0, 0), (1, 0), (1, 1)])
    new = [cases.make_ir(rng, L * N, 2) for _ in filters]
    raw = nr.pack(rng.standard_normal((n, 2)) * 0.2, fin)
    oe = _oracle(L, N, 2, 2, fin, fout, filters, coeffs2=new)
    got = []
    for b in range(n // L):
        if b == sw:
            for f in range(len(filters)):
                oe.set_coeff(f, 2 * f + 1)
        st, r = oe.block(raw[b * L * 16:(b + 1) * L * 16])
        assert st == 0
        got.append(r)
    got = nr.decode(np.concatenate(got), fout, n)
    x = nr.decode(raw, fin, n)
    y0 = nr.convolve(x, filters, 2)
    y1 = nr.convolve(x, [(i, o, h2, si, so) for (i, o, _, si, so), h2 in zip(filters, new)], 2)
    want = nr.switched([y0, y1], [(sw * L, L, 1)])
    assert cases.rel_rms(got, want) <= 1e-12
    assert cases.rel_rms(got[sw * L:(sw + 1) * L], want[sw * L:(sw + 1) * L]) <= 1e-12
    assert cases.rel_rms(want[sw * L:(sw + 1) * L], y1[sw * L:(sw + 1) * L]) > 1e-3     # the fade shows


def test_pack_and_decode_round_trip_every_format():
    rng = np.random.default_rng(7)
    for name, (nb, sb, isf, le) in bo.SAMPLE_FORMATS.items():
        fm = nr.layout([name] * 2, gap=1, order=[1, 0])
        full = 1 << (8 * sb - 1)
        x = rng.standard_normal((50, 2)) * 0.3 if isf else rng.integers(-full, full, (50, 2)).astype(np.float64)
        x[0] = [-full, full - 1] if not isf else [0.5, -0.25]
        back = nr.decode(nr.pack(x, fm), fm, 50, scaled=False)
        if isf and nb == 4:
            x = x.astype(np.float32).astype(np.float64)
        assert np.array_equal(back, x), name
