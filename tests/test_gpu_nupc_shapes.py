"""GPU: the non-uniform partitioned convolver (include/bfhip_nupc.h) against the float64 reference
model (tests/nupc_ref.py), across the shapes its code paths depend on:

  - every transform path a segment engine can take: LDS transforms (L <= 2048), the wave FFT
    (4096, 8192) and the multi-kernel big FFT (16384 and up, to 262144), on the main stream (zero
    slack) and on a background stream (slack), both precisions;
  - schedule shapes: one segment, ratios 2 ... 16, L0 = 4 ... 32 and 4096, taps that end inside a
    partition, on a segment boundary and after one tap, BFHIP_NUPC_BACKGROUND=0;
  - crossbars across the MAC's 8-output groups (8, 9, 17 outputs, up to 10 inputs, sparse and
    doubled pairs, mixed scales);
  - coefficient switches (cross-fade, the split-phase path on a big engine), output gain and
    dither on those shapes;
  - the emit step's output addressing: all 13 sample formats, both byte orders, packed 24 bit,
    gapped frames, mixed formats of one width in one frame, and the same sweep on the inputs;
  - bfhip_nupc_block's overflow[] argument.

Tolerances are the suite's: float32 1e-5 and float64 1e-12 relative RMS over the run, and per L0
block (3x, like test_gpu_nupc.py).  Integer outputs: float64 within 1 LSB with equal overflow
counters; float32 within its rounding noise (the bound of test_random_sample_formats_...).
Impulse probes check placement exactly: nothing before the impulse's block, the scaled taps from
the impulse frame on, and for IRs confined to one segment nothing outside that segment's taps."""
import os

import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_ref as nr

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
DT = {4: np.float32, 8: np.float64}


def sched(L0, lengths, extra=1, last=2):
    """(seg_length, seg_blocks): L0 first, then `lengths`; each segment gets the fewest partitions
    that let the next one start in time, plus `extra` (slack: the next segment runs in the
    background); the last segment gets `last`"""
    seg = [L0] + list(lengths)
    blk, off = [], 0
    for k, L in enumerate(seg):
        if k + 1 == len(seg):
            blk.append(last)
            break
        need = max(1, -(-(seg[k + 1] - L0 - off) // L))
        blk.append(need + extra)
        off += blk[-1] * L
    return seg, blk


def doubling(L0, Lmax, last, two=2):
    seg = []
    L = L0
    while L < Lmax:
        seg.append(L)
        L *= 2
    return seg + [Lmax], [two] * len(seg) + [last]


def offsets(seg):
    off, out = 0, []
    for L, N in zip(*seg):
        out.append(off)
        off += L * N
    return out, off


# name -> (schedule, precisions); the transform path and stream of each segment follow from it:
# L <= 2048 LDS, 4096 / 8192 wave, >= 16384 big; a segment with slack >= L0 (and
# BFHIP_NUPC_BACKGROUND unset) runs on a background stream, one without on the main stream
SCHEDS = {
    "lds": (([64, 128, 256, 512, 1024, 2048], [2, 2, 2, 2, 2, 3]), (4, 8)),
    "wave": (([256, 512, 1024, 2048, 4096, 8192], [2, 2, 2, 2, 2, 2]), (4, 8)),
    "big_main_1024": (([1024, 16384], [15, 2]), (4, 8)),             # zero slack: 16384 on the main stream
    "big_main_64": (([64, 16384], [255, 2]), (4, 8)),
    "big_background": (doubling(64, 16384, 2), (4, 8)),              # 2 x 64 ... 2 x 8192, 16384 x 2
    "big_262144": (doubling(256, 262144, 2), (4, 8)),                # 256 ... 131072, 262144 x 2
    "room_1m_f64": (doubling(256, 65536, 15), (8,)),                 # 1 113 600 taps, IR of 1 048 576
    "ratios_2_4_8_16": (sched(16, [32, 128, 1024, 16384], extra=0, last=1), (4, 8)),
    "L0_4": (sched(4, [8, 32, 128, 512]), (4, 8)),
    "L0_8": (sched(8, [16, 64, 256]), (4, 8)),
    "L0_16": (sched(16, [64, 256, 1024]), (4, 8)),
    "L0_32": (sched(32, [64, 128, 1024, 4096]), (4, 8)),
    "L0_4096": (([4096, 8192, 16384], [2, 2, 2]), (4, 8)),
    "single": (([256], [7]), (4, 8)),
}
PROBE_TAPS = {"room_1m_f64": 1048576}


def path(L):
    return "lds" if L <= 2048 else "wave" if L <= 8192 else "big"


def describe(seg, k, background=True):
    offs, _ = offsets(seg)
    L0, L = seg[0][0], seg[0][k]
    slack = offs[k] - (L - L0)
    bg = background and min(slack, L - L0) >= L0
    return "segment %d (L %d, taps %d..%d, %s FFT, %s stream)" % (
        k, L, offs[k], offs[k] + L * seg[1][k], path(L), "background" if bg else "main")


def flat_ir(rng, n):
    return rng.standard_normal(n) / np.sqrt(n)


def run_nupc(hip, seg, rs, n_in, n_out, filters, raw, n, fin, fout, sets=(), actions=None,
             dither=(), rate=44100, overflow=None, gain=None, safety_limit=0.0):
    """build, finalize and run a convolver; raw: the input stream.  filters: (in, out, taps, si, so);
    sets: per extra set, one IR per filter (add_coeff); actions[b](nu) runs before block call b.
    Returns (raw output stream, convolver, [(block, t_sw)] for every switch the library reported)."""
    nu = hip.Nupc(seg[0], seg[1], rs, n_in, n_out)
    for io, fm in ((0, fin), (1, fout)):
        for c, f in enumerate(fm):
            nu.set_format(io, c, hip.Format(*[getattr(f, k) for k, _ in f._fields_]))
    assert nu.in_bytes == nu.L0 * nr.frame_bytes(fin) and nu.out_bytes == nu.L0 * nr.frame_bytes(fout)
    if safety_limit:
        nu.set_safety_limit(safety_limit)
    if dither:
        nu.enable_dither(list(dither), rate)
    for i, o, h, si, so in filters:
        nu.add_filter(i, o, np.asarray(h, DT[rs]), in_scale=si, out_scale=so)
    for hs in sets:
        for f, h in enumerate(hs):
            nu.add_coeff(f, np.asarray(h, DT[rs]))
    if gain is not None:
        for c, g in enumerate(gain):
            nu.set_output_gain(c, g)
    nu.finalize()
    L0 = nu.L0
    fbi = nr.frame_bytes(fin)
    assert n % L0 == 0
    out, switches, t_last = [], [], -1
    for b in range(n // L0):
        if actions and b in actions:
            actions[b](nu)
        st, r = nu.block(raw[b * L0 * fbi:(b + 1) * L0 * fbi], overflow)
        assert st == 0, b
        out.append(r)
        t = nu.switch_frame()
        if t != t_last:
            switches.append((b, t))
            t_last = t
    return np.concatenate(out), nu, switches


def rounded(filters, rs):
    """the taps the library holds (float32 engines: rounded to float32)"""
    return [(i, o, np.asarray(h, DT[rs]).astype(np.float64), si, so) for i, o, h, si, so in filters]


def level(want):
    """RMS over the frames the output is not silent in (the model's FFT leaves ~1e-17 of round-off
    in silent frames: long runs of them must not dilute the level)"""
    loud = np.abs(want) > 1e-9 * np.abs(want).max()
    return float(np.sqrt((want[loud] ** 2).mean()))


def check_reals(got, want, rs, L0, what="", tol=None):
    """relative RMS over the run and per L0 block (3x; a quiet block against a tenth of the level)"""
    tol = TOL[rs] if tol is None else tol
    assert np.abs(want).max() > 0
    assert cases.rel_rms(got, want) <= tol, (what, cases.rel_rms(got, want))
    floor = 0.1 * level(want)
    for b in range(0, len(want), L0):
        w, g = want[b:b + L0], got[b:b + L0]
        err = float(np.sqrt(((g - w) ** 2).mean()))
        lvl = max(float(np.sqrt((w ** 2).mean())), floor)
        assert err <= 3 * tol * lvl, (what, "block", b // L0, err, lvl)


def check_ints(got, want, rs, what=""):
    d = np.abs(got - want).max(axis=0) if len(got) else 0
    for c in range(got.shape[1]):
        lim = 1 if rs == 8 else 2 + 3e-6 * float(np.abs(want[:, c]).max())
        assert d[c] <= lim, (what, c, d[c], lim)


def check_overflows(nu, of_model, rs, what=""):
    for c, m in enumerate(of_model):
        g = nu.overflow(c)
        if rs == 8:
            assert g.n_overflows == m.n_overflows, (what, c, g.n_overflows, m.n_overflows)
            assert abs(g.intlargest - m.intlargest) <= 1 and g.max == m.max, (what, c)
        else:
            assert abs(g.n_overflows - m.n_overflows) <= max(1, m.n_overflows // 50) and g.max == m.max, (what, c)


# ---------------------------------------------------------------- impulse probes

def _probe_run(hip, name, rs):
    """one convolver per (schedule, precision): 2 inputs; output 0 <- input 0 and output 1 <- input 1
    through flat-noise IRs over the whole schedule (scales 1 / 1 and 0.5 / -0.75), output 2 + k <-
    input 0 through an IR that is non-zero inside segment k's taps only.  Unit impulses on input 0
    at frame L0 - 1 and on input 1 at frame 37 (L0 + 37 when L0 <= 37).  Returns the output, the
    model's and the impulse frames."""
    seg = SCHEDS[name][0]
    offs, total = offsets(seg)
    taps = PROBE_TAPS.get(name, total)
    L0 = seg[0][0]
    rng = np.random.default_rng(len(name) * 100 + rs)
    filters = [(0, 0, flat_ir(rng, taps), 1.0, 1.0), (1, 1, flat_ir(rng, taps), 0.5, -0.75)]
    for k, (L, N) in enumerate(zip(*seg)):
        h = np.zeros(offs[k] + L * N)
        h[offs[k]:] = flat_ir(rng, L * N)
        filters.append((0, 2 + k, h, 1.0, 1.0))
    t = [L0 - 1, 37 if L0 > 37 else L0 + 37]
    n = -(-(max(t) + total + 1) // L0) * L0
    x = np.zeros((n, 2))
    x[t[0], 0] = 1.0
    x[t[1], 1] = 1.0
    fin = nr.layout(["FLOAT64_LE"] * 2)
    fout = nr.layout([FF[rs]] * (2 + len(seg[0])))
    raw, nu, _ = run_nupc(hip, seg, rs, 2, len(fout), filters, nr.pack(x, fin), n, fin, fout)
    nu.close()
    want = nr.convolve(nr.decode(nr.pack(x, fin), fin, n), rounded(filters, rs), len(fout))
    return nr.decode(raw, fout, n), want, t


_PROBE_CACHE = {}


def _probe(hip, name, rs):
    """_probe_run with the default streams, kept for the probes of the same run that follow (the
    parts of one schedule are consecutive test cases)"""
    if (name, rs) not in _PROBE_CACHE:
        _PROBE_CACHE.clear()
        assert "BFHIP_NUPC_BACKGROUND" not in os.environ
        _PROBE_CACHE[(name, rs)] = _probe_run(hip, name, rs)
    return _PROBE_CACHE[(name, rs)]


def _check_probe(got, want, t0, L0, rs, what, support=None):
    """output of a unit impulse at t0: exactly zero in every L0 block before t0's block, zero within
    round-off in that block before t0, the model from t0 on; with support = (a, b) zero within
    round-off outside frames [t0 + a, t0 + b)"""
    b0 = t0 // L0 * L0
    nz = np.flatnonzero(got[:b0])
    assert len(nz) == 0, (what, "non-zero before the impulse's block, frame", int(nz[0]) if len(nz) else None)
    noise = TOL[rs] * level(want)
    assert float(np.abs(got[b0:t0]).max(initial=0)) <= 10 * noise, (what, "output before the impulse")
    if support is not None:
        a, b = t0 + support[0], t0 + support[1]
        outside = np.concatenate([got[:a], got[b:]])
        assert float(np.sqrt((outside ** 2).mean())) <= noise, (what, "output outside the segment's taps")
        big = np.flatnonzero(np.abs(got) > 100 * noise)
        assert big[0] >= a and big[-1] < b, (what, "first / last frame", int(big[0]), int(big[-1]), a, b)
    check_reals(got[t0:], want[t0:], rs, L0, what)


def _probe_parts(name):
    return ["input0", "input1"] + ["seg%d" % k for k in range(len(SCHEDS[name][0][0]))]


PROBES = [(name, rs, part) for name, (_, rss) in SCHEDS.items() for rs in rss for part in _probe_parts(name)]


def _check_part(got, want, t, name, rs, part, background=True):
    seg = SCHEDS[name][0]
    L0 = seg[0][0]
    if part.startswith("input"):
        i = int(part[5:])
        _check_probe(got[:, i], want[:, i], t[i], L0, rs, (name, "impulse on input %d" % i))
        return
    k = int(part[3:])
    offs, _ = offsets(seg)
    _check_probe(got[:, 2 + k], want[:, 2 + k], t[0], L0, rs, (name, describe(seg, k, background)),
                 support=(offs[k], offs[k] + seg[0][k] * seg[1][k]))


@pytest.mark.parametrize("name,rs,part", PROBES, ids=["%s-f%d-%s" % (n, 8 * r, p) for n, r, p in PROBES])
def test_impulse_probe(hip, name, rs, part):
    """unit impulses on one input at a time.  input0 / input1: flat IRs over the whole schedule,
    the output is the scaled taps from exactly the impulse frame (L0 - 1, resp. 37) on.  segK: an
    IR non-zero inside segment K's taps only; its output lies in [t0 + off_K, t0 + off_K + L_K N_K)
    and equals the taps there, so a failure names the segment.  Paths: segment K's FFT path and
    stream as in SCHEDS (the failure message names both); 2 + n_segments outputs, so one MAC group
    (two for the 262144 and 1 M schedules: 13 and 11 outputs)."""
    got, want, t = _probe(hip, name, rs)
    _check_part(got, want, t, name, rs, part)


BG_OFF = ["big_background", "big_262144", "lds", "L0_4"]


@pytest.mark.parametrize("name", BG_OFF)
def test_probes_with_background_streams_off(hip, monkeypatch, name):
    """BFHIP_NUPC_BACKGROUND=0 (set before finalize): every segment on the main stream (zero
    delay_steps), float32, paths as in SCHEDS.  Every probe of test_impulse_probe holds, and the
    output agrees with the default run's within round-off: the ring is accumulated in another
    order, so the bits need not."""
    monkeypatch.setenv("BFHIP_NUPC_BACKGROUND", "0")
    got, want, t = _probe_run(hip, name, 4)
    monkeypatch.delenv("BFHIP_NUPC_BACKGROUND")
    for part in _probe_parts(name):
        _check_part(got, want, t, name, 4, part, background=False)
    ref, _, _ = _probe(hip, name, 4)
    assert cases.rel_rms(got, ref) <= 2 * TOL[4]


# ---------------------------------------------------------------- noise through schedule shapes

def _noise_case(hip, seg, rs, n_in, n_out, filters, n, fin, fout, seed, amp=0.2, **kw):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, n_in))
    for c, f in enumerate(fin):
        v = rng.standard_normal(n) * amp
        x[:, c] = v if f.isfloat else np.round(v / f.scale)
    raw = nr.pack(x, fin)
    got, nu, sw = run_nupc(hip, seg, rs, n_in, n_out, filters, raw, n, fin, fout, **kw)
    xd = nr.decode(raw, fin, n)
    return got, nr.convolve(xd, rounded(filters, rs), n_out), nu, sw, xd


TAP_ENDS = ["full", "mid_partition", "segment_boundary", "one_tap"]


def _tap_lengths(seg):
    offs, total = offsets(seg)
    k = len(offs) - 1 if len(offs) > 1 else 0
    mid = offs[k] + seg[0][k] * max(seg[1][k] - 1, 0) + seg[0][k] // 2 + 3
    boundary = offs[-1] if len(offs) > 1 else seg[0][0] * 3
    return {"full": total, "mid_partition": min(mid, total), "segment_boundary": boundary, "one_tap": 1}


SHAPES = ["ratios_2_4_8_16", "L0_4", "L0_8", "L0_16", "L0_32", "L0_4096", "single"]


@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("name", SHAPES)
def test_schedule_shapes_with_noise(hip, name, rs):
    """noise through a 2-in / 4-out convolver whose four outputs have IRs that end at the last
    tap, inside a partition of the last segment, exactly on the last segment's first tap (it holds
    no taps), and after one tap.  Paths: as in SCHEDS (L0 4 ... 32 on LDS transforms; L0 4096 on
    the wave FFT with a big-FFT last segment; ratios 2, 4, 8, 16); one MAC group."""
    seg = SCHEDS[name][0]
    _, total = offsets(seg)
    lens = _tap_lengths(seg)
    rng = np.random.default_rng(sum(map(ord, name)) + rs)
    filters = []
    for o, end in enumerate(TAP_ENDS):
        for i in range(2):
            filters.append((i, o, flat_ir(rng, lens[end]) / 2,
                            [1.0, 0.5][i], [1.0, -1.0, 0.25, 2.0][o]))
    L0, Lmax = seg[0][0], max(seg[0])
    n = -(-(total + 2 * Lmax) // L0) * L0
    fin = nr.layout(["S24_4LE"] * 2)
    fout = nr.layout([FF[rs]] * 4)
    got, y, _, _, _ = _noise_case(hip, seg, rs, 2, 4, filters, n, fin, fout, seed=rs + len(name))
    got = nr.decode(got, fout, n)
    for o, end in enumerate(TAP_ENDS):
        check_reals(got[:, o], y[:, o], rs, L0, (name, end, lens[end]))


# ---------------------------------------------------------------- crossbars across MAC groups

XBARS = [(3, 8), (10, 9), (5, 17)]
XSCHED = doubling(128, 16384, 1)          # 2 x 128 ... 2 x 8192, 16384 x 1: LDS, wave, big (background)


def _xbar_filters(rng, n_in, n_out, taps):
    filters = []
    for o in range(n_out):
        ins = [i for i in range(n_in) if rng.random() < 0.45] or [int(rng.integers(n_in))]
        for i in ins:
            ln = int(rng.integers(taps // 3, taps + 1))
            filters.append((i, o, flat_ir(rng, ln) / len(ins), float(rng.choice([1.0, -0.5, 2.0])),
                            float(rng.choice([1.0, 0.25, -1.0]))))
    for _ in range(2):                       # two filters on one (in, out) pair
        i, o = filters[int(rng.integers(len(filters)))][:2]
        filters.append((i, o, flat_ir(rng, taps // 2), 0.75, -0.5))
    return filters


@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("n_in,n_out", XBARS)
def test_crossbar_across_mac_groups(hip, n_in, n_out, rs):
    """sparse n_in x n_out crossbars (8 outputs: one full MAC group; 9 and 17: a partial last group,
    so the MAC's summed path), doubled pairs, mixed scales, S24_4LE in; schedule 2 x 128 ... 2 x
    8192 then 16384 x 1 (LDS, wave and big FFT; the big segment on a background stream)"""
    _, total = offsets(XSCHED)
    rng = np.random.default_rng(100 * n_out + n_in + rs)
    filters = _xbar_filters(rng, n_in, n_out, total)
    n = -(-(total + 16384) // 128) * 128
    fin = nr.layout(["S24_4LE"] * n_in)
    fout = nr.layout([FF[rs]] * n_out)
    got, y, _, _, _ = _noise_case(hip, XSCHED, rs, n_in, n_out, filters, n, fin, fout, seed=n_out, amp=0.1)
    got = nr.decode(got, fout, n)
    for o in range(n_out):
        check_reals(got[:, o], y[:, o], rs, 128, ("output", o))


# ---------------------------------------------------------------- switches, gain, dither

def _switch_run(hip, seg, rs, n_in, n_out, n, req_block, F, gains, seed, gain_change=None):
    """every filter switches from set 0 to set 1 at block req_block with an F-frame fade; gains:
    per-output gain from the start; gain_change: (block, channel, gain)"""
    _, total = offsets(seg)
    L0 = seg[0][0]
    rng = np.random.default_rng(seed)
    filters = _xbar_filters(rng, n_in, n_out, total)
    set1 = [flat_ir(rng, total) / 2 for _ in filters]

    def request(nu):
        nu.set_crossfade(F)
        for f in range(len(filters)):
            nu.set_coeff(f, 1)
    acts = {req_block: request}
    if gain_change:
        acts[gain_change[0]] = lambda nu: nu.set_output_gain(gain_change[1], gain_change[2])
    fin = nr.layout([FF[rs]] * n_in)
    fout = nr.layout([FF[rs]] * n_out)
    got, _, nu, sw, xd = _noise_case(hip, seg, rs, n_in, n_out, filters, n, fin, fout, seed, sets=[set1],
                                     actions=acts, gain=gains)
    assert len(sw) == 1 and sw[0][0] == req_block, sw
    t_sw = sw[0][1]
    offs, _ = offsets(seg)
    assert req_block * L0 <= t_sw <= req_block * L0 + max(offs), (t_sw, req_block * L0)
    return got, xd, filters, set1, t_sw, fout


def _switch_model(xd, filters, set1, fout, n, rs, t_sw, F, gains, gain_change, L0):
    """the model's blend at the reported t_sw, times the gains over time"""
    y0 = nr.convolve(xd, rounded(filters, rs), len(fout))
    y1 = nr.convolve(xd, rounded([(i, o, h, si, so) for (i, o, _, si, so), h in zip(filters, set1)], rs), len(fout))
    want = nr.switched([y0, y1], [(t_sw, F, 1)])
    g = np.tile(np.asarray(gains, np.float64), (n, 1))
    if gain_change:
        g[gain_change[0] * L0:, gain_change[1]] = gain_change[2]
    return want * g


@pytest.mark.parametrize("name,rs,n_out,F", [
    ("big_main_1024", 8, 3, 1024 + 77),         # split-phase on a big engine, main stream
    ("big_background", 8, 9, 2 * 64 + 5),      # split-phase on a big engine, background stream
])
def test_switch_on_a_big_fft_segment(hip, name, rs, n_out, F):
    """a cross-faded switch whose window covers blocks of the 16384 segment: that engine runs
    inputs_dev once and mac_dev + outputs_dev under both sets (big FFT, split phase, spectra in the
    convolver's d_z).  Gains 0.5 and -2 on two outputs, one changed mid-run."""
    seg = SCHEDS[name][0]
    L0 = seg[0][0]
    _, total = offsets(seg)
    req = 3 * 16384 // L0 + 5
    n = -(-(req * L0 + total + 2 * 16384) // L0) * L0
    gains = [1.0] * n_out
    gains[0], gains[-1] = 0.5, -2.0
    change = (req + 40, 1, 0.25)
    got, xd, filters, set1, t_sw, fout = _switch_run(hip, seg, rs, 2, n_out, n, req, F, gains, 7, change)
    want = _switch_model(xd, filters, set1, fout, n, rs, t_sw, F, gains, change, L0)
    got = nr.decode(got, fout, n)
    for o in range(n_out):
        check_reals(got[:, o], want[:, o], rs, L0, (name, "output", o, "t_sw", t_sw))


@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("n_out", [9, 17])
def test_crossfade_switch_on_wide_crossbar(hip, n_out, rs):
    """a 5.5-block cross-fade on a 4 x n_out crossbar (partial last MAC group: the MAC's summed
    path into d_z), schedule 2 x 64 ... 2 x 1024, 2048 x 2 (LDS transforms; background and main
    segments), gains != 1 on three outputs"""
    seg = doubling(64, 2048, 2)
    _, total = offsets(seg)
    req, F = 23, 5 * 64 + 32
    n = -(-(req * 64 + 2 * total + 4096) // 64) * 64
    gains = [1.0] * n_out
    gains[1], gains[8], gains[-1] = 0.5, -1.5, 3.0
    change = (req + 3, 8, 0.0)
    got, xd, filters, set1, t_sw, fout = _switch_run(hip, seg, rs, 4, n_out, n, req, F, gains, 11, change)
    want = _switch_model(xd, filters, set1, fout, n, rs, t_sw, F, gains, change, 64)
    got = nr.decode(got, fout, n)
    assert np.all(got[(req + 3) * 64:, 8] == 0)
    for o in range(n_out):
        if o != 8:
            check_reals(got[:, o], want[:, o], rs, 64, ("output", o, "t_sw", t_sw))
    check_reals(got[:(req + 3) * 64, 8], want[:(req + 3) * 64, 8], rs, 64, "output 8 before its gain 0")


def test_one_dithered_output_among_nine_f64(hip):
    """HP-TPDF dither on output 4 of a 3 x 9 S16 crossbar (partial MAC group), the others plain;
    schedule 2 x 64 ... 2 x 512, 1024 x 3 (LDS; background segments), float64: within 1 LSB of
    the model's period-by-period cbuf2raw (a rounding tie moves one sample and the error feedback
    takes it back), overflow counters equal"""
    seg = doubling(64, 1024, 3)
    _, total = offsets(seg)
    rng = np.random.default_rng(3)
    filters = _xbar_filters(rng, 3, 9, total)
    n = -(-(2 * total) // 64) * 64
    fin = nr.layout(["FLOAT64_LE"] * 3)
    fout = nr.layout(["S16_LE"] * 9)
    got, y, nu, _, _ = _noise_case(hip, seg, 8, 3, 9, filters, n, fin, fout, seed=4, dither=[4], rate=300)
    want_raw, of, _ = nr.encode(y, fout, 64, dither=[4], rate=300)
    g, w = nr.ints(got, fout, n), nr.ints(want_raw, fout, n)
    d = np.abs(g - w)
    assert d.max() <= 1 and (d > 0).sum() <= 12, (d.max(), (d > 0).sum())
    plain = nr.ints(nr.encode(y, fout, 64)[0], fout, n)
    assert (plain[:, 4] != w[:, 4]).sum() > n // 4                 # output 4 is dithered
    check_overflows(nu, of, 8)


def test_dither_bit_exact_against_the_oracle_at_nine_outputs(hip):
    """integer-valued float64 inputs through dirac taps (one in the background 512 segment) into
    S16 on 9 outputs, dither on outputs 2 and 8 (the second MAC group): every sample and every
    overflow struct equals the oracle's uniform engine at L = L0 (test_gpu_nupc_dither.py's
    bit-exact setting, widened across the MAC groups)"""
    seg = ([64, 128, 256, 512], [2, 2, 2, 6])
    ch, L0 = 9, 64
    nu = hip.Nupc(seg[0], seg[1], 8, ch, ch)
    nu.set_interleaved(0, "FLOAT64_LE")
    nu.set_interleaved(1, "S16_LE")
    nu.enable_dither([2, 8], 300)
    oe = bo.Engine(L0, 62, 8, ch, ch)
    oe.set_interleaved(0, "FLOAT64_LE")
    oe.set_interleaved(1, "S16_LE")
    assert oe.enable_dither([2, 8], 300)
    for c in range(ch):
        h = np.zeros(1600 + 100 * (c % 3))
        h[0], h[37 + c], h[-1] = 1.0, -1.0, 2.0
        nu.add_filter(c, c, h, out_scale=1.0 / 32768.0)
        oe.add_filter(in_ch=[c], out_ch=[c], coeff=oe.add_coeff(h), out_scale=[1.0 / 32768.0])
    nu.finalize()
    rng = np.random.default_rng(78)
    for b in range(120):
        x = np.round(rng.standard_normal((L0, ch)) * 5000.0)
        x[5, 8] = 40000.0
        gs, g = nu.block(x)
        os_, o = oe.block(x)
        assert gs == os_ == 0
        assert np.array_equal(g.view(np.int16), o.view(np.int16)), b
    for c in range(ch):
        g, o = nu.overflow(c), oe.overflow(c)
        assert (g.n_overflows, g.intlargest, g.max) == (o.n_overflows, o.intlargest, o.max), c


# ---------------------------------------------------------------- sample formats through the emit step

FORMAT_SETS = {
    1: (["S8", "S8"], ["S8", "S8", "S8"]),
    2: (["S16_BE", "S16_LE"], ["S16_LE", "S16_BE", "S16_BE"]),
    3: (["S24_LE", "S24_BE"], ["S24_BE", "S24_LE", "S24_LE"]),
    4: (["S32_BE", "S24_4LE", "FLOAT_BE"], ["S32_LE", "S24_4BE", "FLOAT_LE", "FLOAT_BE", "S24_4LE", "S32_BE"]),
    8: (["FLOAT64_BE", "FLOAT64_LE"], ["FLOAT64_BE", "FLOAT64_LE", "FLOAT64_BE"]),
}


@pytest.mark.parametrize("rs", [4, 8])
@pytest.mark.parametrize("width", sorted(FORMAT_SETS))
def test_sample_formats_gaps_and_byte_orders(hip, width, rs):
    """all 13 formats over the five widths, both byte orders, packed 24 bit; frames with 2 unused
    gap samples and channels in reverse slot order on both sides; width 4 mixes S32, S24_4 and
    FLOAT in one frame.  The last output is 40x louder and clips (integer formats).  Schedule 2 x
    64, 2 x 128, 2 x 256, 6 x 512 (LDS; background segments); the emit step writes every byte."""
    fin_n, fout_n = FORMAT_SETS[width]
    seg = ([64, 128, 256, 512], [2, 2, 2, 6])
    _, total = offsets(seg)
    n_in, n_out = len(fin_n), len(fout_n)
    fin = nr.layout(fin_n, gap=2, order=list(range(n_in))[::-1])
    fout = nr.layout(fout_n, gap=2, order=list(range(n_out))[::-1])
    rng = np.random.default_rng(width * 10 + rs)
    filters = []
    for o in range(n_out):
        for i in range(n_in):
            filters.append((i, o, flat_ir(rng, total - 7 * o) / n_in, 1.0, 40.0 if o == n_out - 1 else 0.5))
    n = 64 * 100
    got_raw, y, nu, _, _ = _noise_case(hip, seg, rs, n_in, n_out, filters, n, fin, fout, seed=width, amp=0.15)
    want_raw, of, _ = nr.encode(y, fout, 64)
    # the gap bytes of the output frames are never written: zero (the wrapper's buffer)
    owned = np.zeros(nr.frame_bytes(fout), bool)
    for f in fout:
        owned[f.byte_offset:f.byte_offset + f.bytes] = True
    assert np.all(got_raw.reshape(n, -1)[:, ~owned] == 0)
    gi, wi = nr.ints(got_raw, fout, n), nr.ints(want_raw, fout, n)
    for c, f in enumerate(fout):
        if f.isfloat:
            tol = TOL[rs] if f.bytes == 8 else max(TOL[rs], 1e-7)
            check_reals(gi[:, c], wi[:, c], rs, 64, (fout_n[c], c), tol=tol)
        else:
            check_ints(gi[:, [c]], wi[:, [c]], rs, (fout_n[c], c))
    check_overflows(nu, of, rs, width)
    assert of[-1].n_overflows > 0                     # the loud output clips (floats: beyond +-1.0)


# ---------------------------------------------------------------- bfhip_nupc_block's overflow[]

@pytest.mark.parametrize("rs", [4, 8])
def test_block_overflow_array_is_read_modified_and_written(hip, rs):
    """overflow[] passed to every block call, starting from non-zero counters: after each call it
    holds the device's counters, which continue from the array's values (read, modified, written
    back like bfhip_engine_block's); a reset of one channel between calls is taken over.  It agrees
    with bfhip_nupc_get_overflow.  S16 out, 3 outputs, the middle one loud enough to clip;
    schedule 2 x 64 ... 2 x 256, 512 x 4 (LDS)."""
    seg = doubling(64, 512, 4)
    _, total = offsets(seg)
    rng = np.random.default_rng(12 + rs)
    filters = [(0, o, flat_ir(rng, total), 1.0, [0.5, 20.0, 1.0][o]) for o in range(3)]
    fin = nr.layout(["FLOAT64_LE"])
    fout = nr.layout(["S16_LE"] * 3)
    start = [bo.Overflow(7 + c, 100 * c, 0.125 * c, 32767.0) for c in range(3)]
    arr = (hip.Overflow * 3)(*[hip.Overflow(*s.astuple()) for s in start])
    n, reset_at = 64 * 60, 30

    def reset(nu):
        assert nu.overflow(1).astuple() == arr[1].astuple()
        arr[1] = hip.Overflow(0, 0, 0.0, 32767.0)
    got, y, nu, _, _ = _noise_case(hip, seg, rs, 1, 3, filters, n, fin, fout, seed=5, overflow=arr,
                                actions={reset_at: reset})
    t = reset_at * 64
    _, of_a, _ = nr.encode(y[:t], fout, 64, overflow=start)
    of_a[1] = bo.Overflow(0, 0, 0.0, 32767.0)
    want_raw, of_b, _ = nr.encode(y[t:], fout, 64, overflow=of_a)
    check_ints(nr.ints(got[t * 6:], fout, n - t), nr.ints(want_raw, fout, n - t), rs)
    assert of_b[1].n_overflows > 0
    for c in range(3):
        assert nu.overflow(c).astuple() == arr[c].astuple(), c
        g, m = arr[c], of_b[c]
        if rs == 8:
            assert (g.n_overflows, g.max) == (m.n_overflows, m.max), c
            assert abs(g.intlargest - m.intlargest) <= 1 and g.largest == pytest.approx(m.largest, rel=1e-9), c
        else:
            assert abs(g.n_overflows - m.n_overflows) <= max(1, m.n_overflows // 50) and g.max == m.max, c
    assert arr[0].n_overflows == 7 and arr[2].n_overflows == 9 and arr[2].intlargest >= 200   # kept the start
