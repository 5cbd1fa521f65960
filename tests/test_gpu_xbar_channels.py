"""The channel stage of the standard crossbar engine (BFHIP_LONG_WINDOW=0) -- sample formats, N:1
maps with integer delay and mute (vchan_in_kernel, vchan_out_kernel), the sub-sample delay FIR
(subdelay_fir_kernel), the HP-TPDF dither pass (dither_kernel), the overflow spread -- held to the
float64 model (xbar_ref.Channels around xbar_ref.Network; tests/test_xbar_channel_model.py pins it to
the oracle) on every FFT path class and across the block lengths at which the FIR starts to tile.

Every case asserts its path through test_gpu_xbar_shapes.run (uses_wave_fft, window_blocks == 2, one
block_mode).  The stage is cases.channel_stage: 0,1,0,1 maps and a 1:1 channel on both sides, packed
S24_LE inputs, member delays 0, 1, L - 1, L, 2L + 3, a muted member a side from block N + 1 on, flat
taps ending mid-partition, 2N + 3 blocks.

    a  maps alone on every path class; float outputs at the suite's 1e-5 / 1e-12 (hold_blocks); one
       case with S16_LE shared outputs, one of them clipping: exact outside the 0.05-LSB band around
       a rounding threshold, 1 LSB inside, overflow records equal on every member
    b  sub-sample filters (sdf_length 31) on a shared input, a raw 1:1 input, a member of a shared
       output beside an unfiltered one and a 1:1 output in place, values 0 (asserted a pure delay),
       +-37, +-99, 12, two run-time changes; both sides of the length at which [history | block]
       leaves one workgroup's LDS (float32 32768 | 65536, float64 16384 | 32768), sdf_length 2047,
       and sdf_length 4096 at 32768 in float64 (tiles shorter than the history); an impulse at
       frame L - 1 through a filtered output gives taps (*) h across the block boundary within
       NOISE * ||h||_2
    c  float64, S16_LE, dither on a 1:1 output and on a shared output behind a sub-sample filter
       (the late pass) at L = 8192 and 65536, the table walk wrapping: within 2 counts, at most
       0.01 % of a channel's samples differ, overflow counts equal

Worst errors of the float32 cases on the MI355X (the XBS lines):
    a  maps, float32          L = 512: 2.6e-7, 4096: 2.9e-7, 8192: 2.9e-7, 16384: 3.0e-7, 65536: 3.2e-7
       S16_LE, L = 16384      501 of 344064 samples differ, all by 1 and inside the band (9.9 % of all)
    b  sdf_length 31          L = 512: 3.1e-7, 4096: 3.4e-7, 8192: 3.3e-7, 16384: 3.5e-7, 32768: 3.5e-7,
                              65536: 3.6e-7; sdf_length 2047 at 32768: 1.4e-6
       impulse, err / ||h||   L = 512: 4.7e-8, 32768: 9.1e-9, 65536: 6.7e-9
(float64: 1.4e-15 ... 1.6e-15, 4.0e-15 with sdf_length 4096, impulses below 1e-16; the dithered
outputs of c equal the model's sample for sample.)  The lengths that fit one tile give what the
untiled kernel gave: its summation order over the taps is unchanged."""
import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_ref as nr
import xbar_ref as xr
from test_gpu_xbar_shapes import NOISE, OUTFMT, flat_ir, hold_blocks, run

pytestmark = pytest.mark.gpu
PATHS = [(512, 4), (512, 8), (4096, 4), (4096, 8), (8192, 4), (8192, 8), (16384, 4), (16384, 8), (65536, 4), (32768, 8)]


def ids(params):
    return ["L%d-rs%d" % p[:2] + ("-sdf%d" % p[2] if len(p) > 2 else "") for p in params]


def stage_case(monkeypatch, L, rs, outfmt, half, N=2, **kw):
    """-> (model, raw input, model's (reals, raw, overflow records, status), engine's raw output, engine)"""
    spec, ch, actions = cases.channel_stage(L, N, rs, outfmt, half, **kw)
    nblk = 2 * N + 3
    model = xr.Channels(spec, ch, cases.subdelay_taps(half, rs) if half else None)
    raw = cases.packed_input(L + rs, nblk * L, model.formats(0), amplitude=0.1)
    want = model.run(raw, nblk, actions)
    return model, nblk, want, (spec, ch, actions, np.split(raw, nblk))


def engine_run(monkeypatch, job, nblk):
    spec, ch, actions, blocks = job
    got, sts, e = run(monkeypatch, spec, blocks, actions, ch=ch)
    assert sts == [0] * nblk
    return got, e


def float_case(monkeypatch, L, rs, half, label, N=2, **kw):
    model, nblk, (y, _, _, status), job = stage_case(monkeypatch, L, rs, OUTFMT[rs], half, N, **kw)
    assert status == [0] * nblk
    got, e = engine_run(monkeypatch, job, nblk)
    e.close()
    return hold_blocks(nr.decode(got, model.formats(1), nblk * L), y, L, rs, "%s L=%d" % (label, L))


# ------------------------------------------------------------------ a. N:1 maps

@pytest.mark.parametrize("L,rs", PATHS, ids=ids(PATHS))
def test_maps_delay_mute_on_every_path(monkeypatch, L, rs):
    float_case(monkeypatch, L, rs, 0, "ch-a", N=2 + (L // 512) % 2)


def test_packed_inputs_shared_integer_outputs_clipping(monkeypatch):
    """S24_LE in, S16_LE out on the multi-kernel transform, float32; physical output 1 (virtual 1
    and 3) clips"""
    L, rs = 16384, 4
    model, nblk, (y, want_raw, ofs, status), job = stage_case(monkeypatch, L, rs, "S16_LE", 0, loud=8.0)
    assert status == [0] * nblk
    u = y * 32768.0 + 0.5
    near = np.abs(u - np.round(u)) < 0.05
    assert near.mean() <= 0.12, near.mean()              # from the model alone, before the device runs
    assert ofs[1].n_overflows > 0 and ofs[0].n_overflows == 0 and ofs[4].n_overflows == 0
    got_raw, e = engine_run(monkeypatch, job, nblk)
    got, want = nr.ints(got_raw, model.formats(1), nblk * L), nr.ints(want_raw, model.formats(1), nblk * L)
    diff = np.abs(got - want)
    print("XBS ch-a S16 L=%d rs=%d differing=%d of %d, in band %.3g, max %d" %
          (L, rs, (diff > 0).sum(), diff.size, near.mean(), diff.max()))
    assert diff[~near].max() == 0 and diff.max() <= 1
    for v in range(5):
        g = e.overflow(v)
        assert (g.n_overflows, g.max) == (ofs[v].n_overflows, ofs[v].max), v
        assert abs(g.intlargest - ofs[v].intlargest) <= 1, v
        if ofs[v].n_overflows:
            assert g.largest == pytest.approx(ofs[v].largest, rel=1e-5), v
    for a, b in ((0, 2), (1, 3)):                         # the members of a group: one record
        assert e.overflow(a).astuple() == e.overflow(b).astuple()
    e.close()


# ------------------------------------------------------------------ b. sub-sample delay

# (L, rs, sdf_length); [history | block] fits one workgroup's LDS up to (32768, 4) and (16384, 8)
SUBDELAY = [p + (31,) for p in PATHS] + [(32768, 4, 31), (32768, 4, 2047), (32768, 8, 4096)]


def test_value_zero_is_a_pure_delay():
    for rs in (4, 8):
        for half in (31, 2047):
            want = np.zeros(2 * half + 1)
            want[half] = 1.0
            assert np.array_equal(cases.subdelay_taps(half, rs)(0), want)


@pytest.mark.parametrize("L,rs,half", SUBDELAY, ids=ids(SUBDELAY))
def test_subsample_delay_on_every_path(monkeypatch, L, rs, half):
    float_case(monkeypatch, L, rs, half, "ch-b sdf=%d" % half)


PROBES = [(512, 4), (512, 8), (32768, 4), (65536, 4), (16384, 8), (32768, 8)]


@pytest.mark.parametrize("L,rs", PROBES, ids=ids(PROBES))
def test_impulse_through_a_filtered_output(monkeypatch, L, rs):
    """a unit impulse at the last frame of block 1 into one filter whose 1:1 output has a sub-sample
    filter (in place): the output is taps (*) h from there on and nothing else, every sample of the
    run within NOISE * ||h||_2"""
    N, half, value = 2, 31, 37
    rng = np.random.default_rng(L + rs)
    h = flat_ir(rng, (N - 1) * L + L // 2 + 1)
    fmt = OUTFMT[rs]
    spec = dict(L=L, N=N, rs=rs, n_in=1, n_out=1, coeffs=[(h, 1.0, 0)], filters=[dict(in_ch=[0], out_ch=[0], coeff=0)])
    ch = dict(in_fmt=fmt, out_fmt=fmt, sdf_length=half, subdelay={(1, 0): value})
    nblk = 2 * N + 3
    x = np.zeros((nblk * L, 1), cases.RAW_NP[fmt])
    t0 = 2 * L - 1
    x[t0, 0] = 1.0
    got_raw, sts, e = run(monkeypatch, spec, np.split(x, nblk), ch=ch, diag=L <= 8192)     # one filter: the one-to-one plan where there is one
    assert sts == [0] * nblk
    e.close()
    got = got_raw.view(cases.RAW_NP[fmt]).astype(np.float64)
    g = np.convolve(h.astype(cases.RAW_NP[fmt]).astype(np.float64), cases.subdelay_taps(half, rs)(value))
    want = np.zeros(nblk * L)
    want[t0:t0 + len(g)] = g[:len(want) - t0]
    norm = np.sqrt((h ** 2).sum())
    err = np.abs(got - want).max() / norm
    print("XBS ch-b impulse L=%d rs=%d err/|h|=%.3g" % (L, rs, err))
    assert err <= NOISE[rs], err


# ------------------------------------------------------------------ c. dither at long blocks

def undefined_dither_samples(L, n_dithered, rate, n_blocks):
    """the samples whose dither the reference reads one element behind its randmap (index r[n] -
    r[n-1] = 255, dither.c:115-130), with the 31 behind each that the error feedback carries it
    into: per dithered channel a boolean [n_blocks * L].  The walk is the oracle's
    (tests/test_gpu_refloop.py names the same samples)"""
    ctx = bo.Ctx(L, 8)
    assert ctx.dither_init(n_dithered, rate)
    tab = ctx.dither_table().astype(np.int64)
    ptr = [int(bo.lib().bfo_dither_randtab_ptr(ctx.h, k)) for k in range(n_dithered)]
    bad = np.zeros((n_dithered, n_blocks * L), bool)
    wraps = [0] * n_dithered
    for b in range(n_blocks):
        for k in range(n_dithered):
            p = ptr[k]
            if p + L >= len(tab):
                tab[0] = tab[p - 1]
                p = 1
                wraps[k] += 1
            seg = tab[p - 1:p + L]
            for i in np.nonzero(seg[1:] - seg[:-1] == 255)[0]:
                bad[k, b * L + int(i):b * L + min(int(i) + 32, L)] = True
            ptr[k] = p + L
    return bad, wraps, len(tab)


@pytest.mark.parametrize("L", [8192, 65536])
def test_dither_at_long_blocks(monkeypatch, L):
    """physical 1: shared, virtual 1 behind a sub-sample filter (the late dither pass); physical 2:
    1:1 and unfiltered (the pass behind the inverse transforms)"""
    rs, N, rate = 8, 2, 300
    model, nblk, (y, want_raw, ofs, status), job = stage_case(monkeypatch, L, rs, "S16_LE", 31, dither=(1, 2), rate=rate,
                                                              loud=4.0, subdelay={(1, 1): 37})
    assert status == [0] * nblk
    bad, wraps, table = undefined_dither_samples(L, 2, rate, nblk)
    assert min(wraps) >= 1 and nblk * L > table, (wraps, table)          # every walk has wrapped
    assert ofs[1].n_overflows > 0
    got_raw, e = engine_run(monkeypatch, job, nblk)
    got, want = nr.ints(got_raw, model.formats(1), nblk * L), nr.ints(want_raw, model.formats(1), nblk * L)
    assert np.array_equal(got[:, 0], want[:, 0])                        # undithered beside them: float64, exact
    for k, p in enumerate((1, 2)):
        diff = np.abs(got[:, p] - want[:, p])[~bad[k]]
        print("XBS ch-c L=%d rs=%d out=%d differing=%d of %d, max %d, left out %d" %
              (L, rs, p, (diff > 0).sum(), diff.size, diff.max(), bad[k].sum()))
        assert diff.max() <= 2, (p, diff.max())
        assert (diff > 0).mean() <= 1e-4, (p, (diff > 0).mean())
    for v in range(5):
        assert e.overflow(v).n_overflows == ofs[v].n_overflows, v
    e.close()
