"""GPU: HP-TPDF dither on the integer outputs of the non-uniform convolver
(bfhip_nupc_enable_dither, include/bfhip_nupc.h).  The reference dithers in convolver_cbuf2raw
(dither_funs.h:7-69) once per period; with a period of L0 frames the nupc must produce exactly
that.  References: the oracle's uniform engine with L = L0 and the same enable_dither call, or
float64 numpy convolutions requantised period by period with the oracle's cbuf2raw."""
import ctypes as C

import numpy as np
import pytest

import bforacle as bo
import cases

pytestmark = pytest.mark.gpu
SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])     # offsets 0, 128, 384, 896; 3968 taps
EINVAL, ESTATE = -1, -5


def _nupc(hip, rs, n_ch, outfmt, infmt=None, sched=SMALL, dither=None, rate=300, max_size=0):
    nu = hip.Nupc(sched[0], sched[1], rs, n_ch, n_ch)
    nu.set_interleaved(0, infmt or ("FLOAT_LE" if rs == 4 else "FLOAT64_LE"))
    nu.set_interleaved(1, outfmt)
    if dither:
        nu.enable_dither(dither, rate, max_size)
    return nu


def _conv(x, h, n):
    m = len(x) + len(h) - 1
    nfft = 1 << (m - 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x, nfft) * np.fft.rfft(h, nfft), nfft)[:n]


def _requantise(y, outfmt, dither, rate, L0=64):
    """y: [frames][n_out] reals in output units (1/scale applied); the reference's cbuf2raw per
    L0-frame period, dither slot = rank among the dithered outputs.  Returns the integers and the
    overflow structs."""
    n, n_out = y.shape
    nbytes, sbytes = bo.SAMPLE_FORMATS[outfmt][:2]
    ctx = bo.Ctx(L0, 8)
    assert ctx.dither_init(len(dither), rate)
    fmts = bo.interleaved_formats(outfmt, n_out)
    full = float(1 << (8 * sbytes - 1))
    ofs = [bo.Overflow(0, 0, 0.0, full - 1) for _ in range(n_out)]
    out = []
    for b in range(n // L0):
        raw = np.zeros(L0 * n_out * nbytes, np.uint8)
        for c in range(n_out):
            d = dither.index(c) if c in dither else -1
            st, r = ctx.cbuf2raw(y[b * L0:(b + 1) * L0, c], fmts[c], len(raw), ofs[c], dither_channel=d)
            assert st == 0
            raw += r
        out.append(raw)
    return _ints(np.concatenate(out), outfmt, n_out), ofs


def _ints(raw, outfmt, n_out):
    nbytes = bo.SAMPLE_FORMATS[outfmt][0]
    dt = {2: np.int16, 4: np.int32}[nbytes]
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), dt).reshape(-1, n_out).astype(np.int64)


def _close(got, want, max_diff=12):
    """equal but for rounding ties: a tie moves one sample by 1 LSB and the error feedback undoes it
    within the next two samples"""
    d = np.abs(got - want)
    assert d.max() <= 1, d.max()
    assert (d > 0).sum() <= max_diff, (d > 0).sum()


def test_bit_exact_against_the_reference_dither_f64(hip):
    """integer-valued f64 input through diracs (one in a background segment) to S16, dither on
    outputs 0 and 2 with a 6001-byte table (each walk wraps every ~47 periods): every sample,
    the error feedback across periods and the overflow structs equal the oracle's uniform engine
    at L = L0.  Some samples clip."""
    ch, L0 = 3, 64
    nu = _nupc(hip, 8, ch, "S16_LE", dither=[0, 2])
    oe = bo.Engine(L0, 62, 8, ch, ch)
    oe.set_interleaved(0, "FLOAT64_LE")
    oe.set_interleaved(1, "S16_LE")
    assert oe.enable_dither([0, 2], 300)
    for c in range(ch):
        h = np.zeros(1600 + 100 * c)
        h[0], h[37 + c], h[-1] = 1.0, -1.0, 2.0                   # taps 0, 37.., 1599.. (512 segment)
        nu.add_filter(c, c, h, out_scale=1.0 / 32768.0)
        oe.add_filter(in_ch=[c], out_ch=[c], coeff=oe.add_coeff(h), out_scale=[1.0 / 32768.0])
    nu.finalize()
    rng = np.random.default_rng(77)
    for b in range(300):
        x = np.round(rng.standard_normal((L0, ch)) * 5000.0)
        x[5, 0] = 40000.0
        x[9, 2] = -50000.0
        gs, g = nu.block(x)
        os_, o = oe.block(x)
        assert gs == os_ == 0
        assert np.array_equal(g.view(np.int16), o.view(np.int16)), b
    for c in range(ch):
        g, o = nu.overflow(c), oe.overflow(c)
        assert (g.n_overflows, g.intlargest, g.max) == (o.n_overflows, o.intlargest, o.max), c
        assert g.largest == pytest.approx(o.largest, rel=1e-12)
        if c != 1:
            assert g.n_overflows > 0


def test_f32_within_one_lsb(hip):
    ch, L0 = 2, 64
    nu = _nupc(hip, 4, ch, "S16_LE", infmt="S24_4LE", dither=[0, 1], rate=44100)
    oe = bo.Engine(L0, 62, 4, ch, ch)
    oe.set_interleaved(0, "S24_4LE")
    oe.set_interleaved(1, "S16_LE")
    assert oe.enable_dither([0, 1], 44100)
    for c in range(ch):
        h = cases.make_ir(np.random.default_rng(60 + c), nu.taps, 1).astype(np.float32)
        nu.add_filter(c, c, h)
        oe.add_filter(in_ch=[c], out_ch=[c], coeff=oe.add_coeff(h))
    nu.finalize()
    for blk in cases.raw_blocks(9, 120, L0, ch, "S24_4LE", amplitude=0.3):
        gs, g = nu.block(blk)
        os_, o = oe.block(blk)
        assert gs == os_ == 0
        d = np.abs(g.view(np.int16).astype(int) - o.view(np.int16).astype(int))
        assert d.max() <= 2 and (d > 0).mean() < 0.05


def test_dither_follows_crossfade_switch_and_gain_f64(hip):
    """a cross-faded switch, a gain change and a mute on dithered outputs: the dither input is the
    blended value times the gain times 1/scale; gain 0 is dithered silence"""
    L0, n_blk = 64, 140
    nu = _nupc(hip, 8, 2, "S16_LE", dither=[0, 1])
    rng = np.random.default_rng(5)
    h = [[rng.standard_normal(nu.taps) / np.sqrt(nu.taps) for _ in range(2)] for _ in range(2)]
    for c in range(2):
        nu.add_filter(c, c, h[c][0])
        assert nu.add_coeff(c, h[c][1]) == 1
    nu.finalize()
    x = rng.standard_normal((n_blk * L0, 2)) * 0.2
    gain = np.ones((n_blk * L0, 2))
    got, t_sw = [], None
    for b in range(n_blk):
        if b == 12:
            nu.set_crossfade(150)
            nu.set_coeff(0, 1)
            nu.set_coeff(1, 1)
        for bb, c, g in ((30, 0, 0.5), (50, 1, 0.0), (70, 1, 1.5)):
            if b == bb:
                nu.set_output_gain(c, g)
                gain[b * L0:, c] = g
        st, raw = nu.block(x[b * L0:(b + 1) * L0])
        assert st == 0
        got.append(raw)
        if nu.switch_frame() != -1 and t_sw is None:
            t_sw = nu.switch_frame()
    assert t_sw is not None and 12 * L0 <= t_sw
    n = len(x)
    want = np.zeros((n, 2))
    for c in range(2):
        yo, yn = _conv(x[:, c], h[c][0], n), _conv(x[:, c], h[c][1], n)
        y = yo.copy()
        y[t_sw:] = yn[t_sw:]
        j = np.arange(150)
        w = j / 149.0
        y[t_sw:t_sw + 150] = (1 - w) * yo[t_sw:t_sw + 150] + w * yn[t_sw:t_sw + 150]
        want[:, c] = y
    want = want * gain * 32768.0
    ref, _ = _requantise(want, "S16_LE", [0, 1], 300)
    g = _ints(np.concatenate(got), "S16_LE", 2)
    _close(g, ref)
    mute = g[50 * L0:70 * L0, 1]
    assert np.abs(mute).max() <= 3 and np.any(mute != 0)          # dithered silence, not zeros


def test_status_bits_come_with_the_block_that_made_them(hip):
    """an over-limit and a NaN sample on the dithered output 1 (output 0 is not dithered): the bit
    is in the return value of that very block call, and the next call is clean again"""
    L0 = 64
    nu = _nupc(hip, 8, 2, "S16_LE", dither=[1])
    assert hip.lib().bfhip_nupc_set_safety_limit(nu.h, 2.0) == 0
    for c in range(2):
        nu.add_filter(c, c, np.array([1.0]))
    nu.finalize()
    sts = []
    for b in range(12):
        x = np.full((L0, 2), 0.25)
        if b == 5:
            x[10, 1] = 3.0                                         # 98304 > 2 * 32767
        if b == 9:
            x[3, 1] = np.nan
        sts.append(nu.block(x)[0])
    assert sts[:5] == [0] * 5 and sts[6:9] == [0] * 3, sts
    assert sts[5] == hip.ST_SAFETY, sts
    assert sts[9] & hip.ST_NONFINITE, sts


def test_block_and_block_dev_same_bits(hip):
    import torch
    L0, n_blk = 64, 60
    runs = []
    for dev in (False, True):
        nu = _nupc(hip, 4, 2, "S16_LE", dither=[0, 1], rate=1000)
        rng = np.random.default_rng(3)
        for c in range(2):
            nu.add_filter(c, c, (rng.standard_normal(nu.taps) / np.sqrt(nu.taps)).astype(np.float32))
            assert nu.add_coeff(c, (rng.standard_normal(nu.taps) / np.sqrt(nu.taps)).astype(np.float32)) == 1
        nu.finalize()
        x = (rng.standard_normal((n_blk * L0, 2)) * 0.2).astype(np.float32)
        out = []
        if dev:
            din = torch.empty(L0 * 2 * 4, dtype=torch.uint8, device="cuda")
            dout = torch.empty(L0 * 2 * 2, dtype=torch.uint8, device="cuda")
        for b in range(n_blk):
            if b == 9:
                nu.set_crossfade(100)
                nu.set_coeff(0, 1)
                nu.set_coeff(1, 1)
            if b == 15:
                nu.set_output_gain(1, 0.25)
            xb = x[b * L0:(b + 1) * L0]
            if dev:
                din.copy_(torch.from_numpy(xb.view(np.uint8).ravel().copy()))
                torch.cuda.synchronize()
                nu.block_dev(din, dout)
                assert nu.sync() == 0
                out.append(dout.cpu().numpy().copy())
            else:
                st, raw = nu.block(xb)
                assert st == 0
                out.append(raw)
        runs.append(np.concatenate(out))
    assert np.array_equal(runs[0], runs[1])


def test_undithered_output_is_unchanged(hip):
    L0, n_blk = 64, 50
    outs = []
    for dither in (None, [1]):
        nu = _nupc(hip, 4, 2, "S16_LE", dither=dither, rate=44100)
        for c in range(2):
            nu.add_filter(c, c, cases.make_ir(np.random.default_rng(8 + c), nu.taps, 1).astype(np.float32))
        nu.finalize()
        x = (np.random.default_rng(4).standard_normal((n_blk * L0, 2)) * 0.3).astype(np.float32)
        outs.append(_ints(np.concatenate([nu.block(x[b * L0:(b + 1) * L0])[1] for b in range(n_blk)]), "S16_LE", 2))
    assert np.array_equal(outs[0][:, 0], outs[1][:, 0])
    assert not np.array_equal(outs[0][:, 1], outs[1][:, 1])


def test_argument_and_state_errors(hip):
    nu = hip.Nupc(*SMALL, 4, 2, 2)
    with pytest.raises(hip.BfhipError, match="floating point"):
        nu.enable_dither([0], 48000)                               # outputs are FLOAT_LE by default
    nu.set_interleaved(1, "S16_LE")
    for chs in ([1, 0], [0, 0], [2], [-1]):
        with pytest.raises(hip.BfhipError):
            nu.enable_dither(chs, 48000)
    with pytest.raises(hip.BfhipError):
        nu.enable_dither([0], 0)
    with pytest.raises(hip.BfhipError, match="too small"):
        nu.enable_dither([0, 1], 48000, max_size=1000)
    nu.enable_dither([0, 1], 48000)
    nu.add_filter(0, 0, np.ones(8, np.float32))
    nu.finalize()
    arr = (C.c_int * 1)(0)
    assert hip.lib().bfhip_nupc_enable_dither(nu.h, arr, 1, 48000, 0) == ESTATE
    # a format set to float after enable_dither is refused at finalize
    nf = hip.Nupc(*SMALL, 4, 1, 1)
    nf.set_interleaved(1, "S16_LE")
    nf.enable_dither([0], 48000)
    nf.set_interleaved(1, "FLOAT_LE")
    nf.add_filter(0, 0, np.ones(8, np.float32))
    with pytest.raises(hip.BfhipError, match="floating point"):
        nf.finalize()


def test_room_correction_dithered_s24_float64(hip):
    """BASELINE configs[4]: 2-in/2-out crossbar, 1048576-tap filters, float64, 64-frame latency,
    S24_4LE out with both outputs dithered, 512 periods against float64 numpy convolutions
    requantised by the reference's cbuf2raw"""
    seg_len, k = [], 64
    while k < 8192:
        seg_len.append(k)
        k *= 2
    covered = 2 * sum(seg_len)
    sched = (seg_len + [8192], [2] * len(seg_len) + [-(-(1048576 - covered) // 8192)])
    L0, n = 64, 4 * 8192
    nu = _nupc(hip, 8, 2, "S24_4LE", sched=sched, dither=[0, 1], rate=48000)
    rng = np.random.default_rng(41)
    h = [[cases.make_ir(rng, 1048576, 2) for _ in range(2)] for _ in range(2)]
    for o in range(2):
        for i in range(2):
            nu.add_filter(i, o, h[o][i], out_scale=-1.0 if o else 1.0)
    nu.finalize()
    x = rng.standard_normal((n, 2)) * 0.3
    got = []
    for b in range(n // L0):
        st, raw = nu.block(x[b * L0:(b + 1) * L0])
        assert st == 0
        got.append(raw)
    want = np.zeros((n, 2))
    for o in range(2):
        for i in range(2):
            want[:, o] += _conv(x[:, i], h[o][i][:n], n) * (-1.0 if o else 1.0)
    ref, _ = _requantise(want * 8388608.0, "S24_4LE", [0, 1], 48000)
    g = _ints(np.concatenate(got), "S24_4LE", 2)
    assert np.abs(ref).max() > 1000
    _close(g, ref)
