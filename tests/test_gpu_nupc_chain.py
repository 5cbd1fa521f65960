"""GPU: the non-uniform convolver's whole per-period chain (include/bfhip_nupc.h) against the float64
chain model of tests/nupc_chain_ref.py (checked on its own in tests/test_nupc_chain_model.py):

    input    mute -> raw delay line -> raw to real -> sub-delay FIR
    middle   segment blocks under one or two assignments, blended per segment or over their sum
    output   x gain(frame) / scale -> sub-delay FIR -> quantise or dither -> raw delay line -> mute

A. the sub-delay FIR's loops that the per-feature tests never enter: filter block sizes above 256
   (more than one history sample per thread), bs == tile, periods of more than one 2048-frame tile.
B. the delay kernel with more than one sample per thread: L0 256, 512, 4096.
C. staggered switches with everything behind the ring switched on, on the LDS, wave-FFT and big-FFT
   paths, with more than 8 outputs.
D. seeded sessions that make every kind of call in one run.

Bars (the project's): float outputs relative RMS 1e-5 (float32) / 1e-12 (float64) per channel over
the run and 3x that per L0 block; integer outputs within one count of the model (float64, or float32
at 16 bits) with equal overflow counters; dithered outputs equal but for rounding ties (at most 12
samples one count off, test_gpu_nupc_dither.py's _close); bytes where device meets device.  The
per-block bar is check_reals' of tests/test_gpu_nupc_shapes.py with a lower floor: a block is
measured against its own level or, where that is lower, against 1 % of the run's level (there: 10 %),
since a block that holds only the first ripples of a filter or the end of a mute carries its
neighbours' rounding error."""
import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_chain_ref as cr
import nupc_ref as nr
import nupc_stagger_ref as sr
from nupc_chain_ref import IN, OUT, STAGGERED

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
SMALL = sr.SMALL
WAVE = ([256, 512, 1024, 2048, 4096], [2] * 5)      # the wave FFT path
BIGS = ([1024, 16384], [15, 2])                     # a big FFT on the main stream (zero slack)


def _raw(rng, fmt, frames, n_ch, amp=0.1):
    """random raw frames; no sample is exactly zero"""
    nbytes, sbytes, isfloat, _ = bo.SAMPLE_FORMATS[fmt]
    x = rng.standard_normal((frames, n_ch)) * amp
    if isfloat:
        return x.astype(np.float32 if nbytes == 4 else np.float64).view(np.uint8).reshape(frames, -1)
    full = 1 << (8 * sbytes - 1)
    v = np.clip(np.round(x * full), -full, full - 1)
    v[v == 0] = 1
    v = v.astype("<i8")
    return np.ascontiguousarray(v.view(np.uint8).reshape(frames, n_ch, 8)[:, :, :nbytes]).reshape(frames, -1)


def _device(hip, ch, reserve_gain=False):
    """the convolver a Chain describes"""
    dt = np.float32 if ch.rs == 4 else np.float64
    nu = hip.Nupc(ch.sched[0], ch.sched[1], ch.rs, ch.n_in, ch.n_out)
    assert nu.taps == ch.taps
    nu.set_interleaved(IN, ch.names[IN])
    nu.set_interleaved(OUT, ch.names[OUT])
    if ch.dither:
        nu.enable_dither(list(ch.dither), ch.rate)
    if ch.half:
        nu.enable_subdelay(ch.half)
    for io in (IN, OUT):
        for c, v in ch.sub0[io].items():
            nu.set_subdelay(io, c, v)
        for c, (init, maxd) in ch.delay[io].items():
            nu.set_maxdelay(io, c, maxd)
            nu.set_delay(io, c, init)
    for f, (i, o, si, so) in enumerate(ch.filters):
        nu.add_filter(i, o, ch.h[f][0].astype(dt), in_scale=si, out_scale=so)
        for j in range(1, len(ch.h[f])):
            assert nu.add_coeff(f, ch.h[f][j].astype(dt)) == j
    if reserve_gain:
        nu.reserve_filter_gain()
    nu.finalize()
    return nu


def _taps(rng, n, dt, n_sets):
    """flat noise over the whole schedule in the convolver's precision, as float64"""
    return [(rng.standard_normal(n) / np.sqrt(n)).astype(dt).astype(np.float64) for _ in range(n_sets)]


def _check(section, got_raw, res, ch, periods, nu=None, status=None):
    """the bars of the module docstring on the raw output; with nu the overflow structs, with
    status the status words"""
    n, L0, rs = periods * ch.L0, ch.L0, ch.rs
    fm = ch.fmts[OUT]
    if fm[0].isfloat:
        g, w = nr.decode(got_raw, fm, n), nr.decode(res.raw, fm, n)
        floor = 0.01 * np.sqrt(np.mean(w * w, axis=0))
        for c in range(ch.n_out):
            err = cases.rel_rms(g[:, c], w[:, c])
            gb, wb = g[:, c].reshape(-1, L0), w[:, c].reshape(-1, L0)
            eb = np.sqrt(np.mean((gb - wb) ** 2, axis=1)) / np.maximum(np.sqrt(np.mean(wb * wb, axis=1)), floor[c])
            print("%s rs %d ch %d: rel rms %.3g, worst block %.3g" % (section, rs, c, err, eb.max()))
            assert err <= TOL[rs], (c, err)
            assert eb.max() <= 3 * TOL[rs], (c, int(eb.argmax()), eb.max())
    else:
        d = np.abs(nr.ints(got_raw, fm, n) - nr.ints(res.raw, fm, n))
        print("%s rs %d: max count difference %d, samples off per channel %s" % (section, rs, d.max(), (d > 0).sum(axis=0)))
        assert d.max() <= 1, d.max()
        if ch.dither:
            off = (d[:, list(ch.dither)] > 0).sum()
            print("frames off on the dithered channels: %s" % np.nonzero(d[:, list(ch.dither)].max(axis=1))[0][:16])
            assert off <= 12, off
    if status is not None:
        assert list(status) == list(res.status)
    if nu is not None:
        for c in range(ch.n_out):
            of, w = nu.overflow(c), res.overflow[c]
            assert of.n_overflows == w.n_overflows, (c, of.n_overflows, w.n_overflows)
            assert of.max == w.max
            if rs == 8:
                assert of.intlargest == w.intlargest and of.largest == pytest.approx(w.largest, rel=1e-9), c
            else:
                assert of.largest == pytest.approx(w.largest, rel=1e-4), c


def _blocks(nu, x, L0, periods, before=None, after=None):
    out, sts = [], []
    for p in range(periods):
        if before:
            before(p)
        st, y = nu.block(x[p * L0:(p + 1) * L0])
        sts.append(st)
        out.append(y)
        if after:
            after(p)
    return np.concatenate(out), sts


# ---------------------------------------------------------------- A. sub-delay loop ranges

def _sd_filters(ch, rng, dt):
    n = ch.taps
    for o in range(3):
        for i in (o, (o + 1) % 3):
            ch.add_filter(i, o, _taps(rng, n, dt, 1))


@pytest.mark.parametrize("rs,sched,half,infmt,outfmt,dither", [
    (4, ([512], [2]), 128, None, None, ()),                        # bs 512: keep[1]
    (8, ([512], [2]), 128, None, None, ()),
    (4, ([1024], [2]), 511, None, None, ()),                       # bs 1024 == tile, keep[3]
    (8, ([1024], [2]), 511, None, None, ()),
    (4, ([2048], [2]), 300, None, None, ()),                       # one full tile
    (8, ([2048], [2]), 300, "S24_LE", None, ()),
    (4, ([4096], [2]), 31, None, None, ()),                        # two tiles, bs 64
    (8, ([4096], [2]), 31, None, "S16_LE", (0, 1, 2)),
    (4, ([4096], [2]), 511, None, None, ()),                       # two tiles, bs 1024
    (8, ([4096], [2]), 511, None, None, ()),
    (4, ([8192], [2]), 255, None, None, ()),                       # four tiles, bs 512
    (8, ([8192], [2]), 255, None, None, ()),
    (4, ([1024, 2048], [2, 2]), 511, None, None, ()),              # a second segment reads the ring of reals
])
def test_subdelay_loop_ranges(hip, rs, sched, half, infmt, outfmt, dither):
    """three channels per side: 0 with a filter whose value changes at periods 2 and 4 (37, -99,
    99 on the inputs, -99, 99, -25 on the outputs), 1 with value 0, 2 without a filter (sdf_length
    frames through its line).  Fractional values against the chain model; then the same convolver
    with every filter at 0 against a twin with integer delays, byte for byte (not with dither: the
    twin's delay sits behind the dither chain, the filter in front of it)."""
    dt = np.float32 if rs == 4 else np.float64
    infmt, outfmt = infmt or FF[rs], outfmt or FF[rs]
    L0 = sched[0][0]
    periods = 8
    plan = {IN: (37, -99, 99), OUT: (-99, 99, -25)}

    def chain(zero):
        ch = cr.Chain(sched, rs, 3, 3, infmt, outfmt, half=half, dither=dither)
        _sd_filters(ch, np.random.default_rng(half + L0), dt)
        for io in (IN, OUT):
            ch.subdelay(io, 0, 0 if zero else plan[io][0])
            ch.subdelay(io, 1, 0)
        return ch

    x = _raw(np.random.default_rng(rs + half), infmt, periods * L0, 3)
    ch = chain(False)
    nu = _device(hip, ch)

    def before(p):
        if p in (2, 4):
            for io in (IN, OUT):
                nu.set_subdelay(io, 0, plan[io][p // 2])
                ch.set_subdelay(p, io, 0, plan[io][p // 2])

    got, sts = _blocks(nu, x, L0, periods, before)
    assert not any(sts)
    assert (nu.get_subdelay(IN, 0), nu.get_subdelay(OUT, 0), nu.get_subdelay(IN, 2)) == (99, -25, -100)
    _check("A", got, ch.render(x, periods), ch, periods, nu)
    nu.close()
    if dither:
        return
    a = _device(hip, chain(True))
    tw = cr.Chain(sched, rs, 3, 3, infmt, outfmt)
    _sd_filters(tw, np.random.default_rng(half + L0), dt)
    for io in (IN, OUT):
        for c in range(3):
            tw.line(io, c, half, -1)
    b = _device(hip, tw)
    ya, sa = _blocks(a, x, L0, periods)
    yb, sb = _blocks(b, x, L0, periods)
    assert sa == sb and not any(sa)
    assert ya.any() and np.array_equal(ya, yb)


# ---------------------------------------------------------------- B. delay kernel above 256 frames

@pytest.mark.parametrize("fmt", ["S16_LE", "S24_LE", "S32_LE", "FLOAT64_LE"])       # 2, 3, 4 and 8 bytes
@pytest.mark.parametrize("L0", [256, 512, 4096])
def test_delay_kernel_with_several_samples_per_thread(hip, L0, fmt):
    """six channels per side with delays 1, L0 - 1, L0, L0 + 1, 3 L0 + 7 and maxdelay; channels 0
    and 5 change at run time across the L0 boundary in both directions (short <-> whole fragments,
    with change_delay's zero-fills), a value above maxdelay is ignored, and a mute comes and goes on
    both sides.  The bar of test_gpu_nupc_delay.py: the bytes of a plain convolver fed the model's
    input, with the model applied to its output."""
    rs = 8 if fmt == "FLOAT64_LE" else 4
    n_ch, periods, maxd = 6, 26, 4 * L0 + 3
    spec = [(1, maxd), (L0 - 1, -1), (L0, L0), (L0 + 1, -1), (3 * L0 + 7, -1), (maxd, maxd)]
    sched = ([L0], [2])
    rng = np.random.default_rng(L0 + len(fmt))
    nus = []
    for _ in range(2):
        nu = hip.Nupc(sched[0], sched[1], rs, n_ch, n_ch)
        nu.set_interleaved(IN, fmt)
        nu.set_interleaved(OUT, fmt)
        nus.append(nu)
    r2 = np.random.default_rng(5)
    for o in range(n_ch):
        h = r2.standard_normal(2 * L0) * np.exp(-np.arange(2 * L0) / 100.0) / 6.0
        for nu in nus:
            nu.add_filter(o, o, h)
    a, b = nus
    for io in (IN, OUT):
        for c, (d, m) in enumerate(spec):
            a.set_maxdelay(io, c, m)
            a.set_delay(io, c, d)
    a.finalize()
    b.finalize()
    mi, mo = cr.Model(IN, fmt, spec, L0), cr.Model(OUT, fmt, spec, L0)
    plan = {3: [("d", 0, L0 + 1)],                     # short -> whole fragments: zero-fill
            5: [("m", 1, True), ("d", 5, L0)],         # whole -> short, from maxdelay
            8: [("d", 0, L0 - 1)],                     # whole -> short
            10: [("d", 5, 3 * L0 + 7), ("m", 4, True)],
            12: [("d", 0, maxd + 1), ("m", 1, False)],  # above maxdelay: ignored
            13: [("d", 0, maxd)],
            16: [("d", 0, L0), ("d", 5, 1), ("m", 4, False)],
            19: [("d", 0, 2 * L0), ("d", 5, L0 + 1)],
            22: [("d", 0, 0), ("d", 5, maxd)]}
    x = _raw(rng, fmt, periods * L0, n_ch, 0.3)
    for p in range(periods):
        for kind, c, v in plan.get(p, ()):
            for io, m in ((IN, mi), (OUT, mo)):
                if kind == "d":
                    a.set_delay(io, c, v)
                    m.lines[c].req = v
                else:
                    a.set_mute(io, c, v)
                    m.lines[c].muted = v
        xb = x[p * L0:(p + 1) * L0]
        sa, ya = a.block(xb)
        sb, yb = b.block(mi.run(xb))
        assert sa == sb == 0
        assert np.array_equal(ya, mo.run(yb)), p
        for io, m in ((IN, mi), (OUT, mo)):
            assert [a.get_delay(io, c) for c in range(n_ch)] == [ln.cur for ln in m.lines], (p, io)
    assert ya.any()
    assert mi.lines[0].cur == 0 and mi.lines[5].cur == maxd


# ---------------------------------------------------------------- C. staggered switches through the chain

_C_CACHE = {}


def _c_cache(key):
    """the model's per-filter segment outputs of one schedule and precision, shared by the cases that
    follow each other with the same key (every F and output format: the input side's calls do not
    depend on them); one key's are held at a time.  The Chain files each array under the digests of
    the samples and taps it was computed from, so a case that draws something else computes afresh."""
    if key not in _C_CACHE:
        _C_CACHE.clear()
        _C_CACHE[key] = {}
    return _C_CACHE[key]


C_SCHEDS = {"small": SMALL, "wave": WAVE, "big": BIGS}
# the whole matrix: every schedule x F in {0, 2, L0, 700} (and 20000, longer than any segment block,
# on the big one) x {float32, float64, S24_4LE at float64, dithered S16_LE at float64, S16_LE at
# float32}, ordered so that the cases of one (schedule, precision) follow each other
C_CASES = [(name, F, rs, outfmt, dither)
           for name in C_SCHEDS
           for rs, outfmt, dither in ((4, None, ()), (4, "S16_LE", ()), (8, None, ()), (8, "S24_4LE", ()),
                                      (8, "S16_LE", (1, 4, 8)))
           for F in (0, 2, C_SCHEDS[name][0][0], 700) + ((20000,) if name == "big" else ())]


@pytest.mark.parametrize("name,F,rs,outfmt,dither", C_CASES,
                         ids=["%s-F%d-rs%d-%s%s" % (n, F, rs, o or "float", "-dither" if d else "") for n, F, rs, o, d in C_CASES])
def test_staggered_switch_through_the_chain(hip, name, F, rs, outfmt, dither):
    """a 3 x 9 crossbar (more than 8 outputs), two sets per filter.  The first commit switches every
    filter's set and one gain; the second, issued as soon as switch_busy() clears, is gain-only on
    some filters and back to set 0 on others.  An output gain ramp starts one period before the
    first commit and ends inside its fade (F < 4: right behind it); output 1 has a sub-delay filter
    and a delay line, output 2 a line that changes, input 0 a delay that changes.  F = 20000 is
    longer than any segment block."""
    dt = np.float32 if rs == 4 else np.float64
    outfmt = outfmt or FF[rs]
    sched = C_SCHEDS[name]
    L0, Lmax = sched[0][0], sched[0][-1]
    n_in, n_out, half = 3, 9, 15
    ch = cr.Chain(sched, rs, n_in, n_out, FF[rs], outfmt, half=half, dither=dither, cache=_c_cache((name, rs)))
    rng = np.random.default_rng(len(name))
    for o in range(n_out):
        for i in range(n_in):
            ch.add_filter(i, o, _taps(rng, ch.taps, dt, 2), in_scale=(1.0, 0.5, -1.0)[i], out_scale=1.0 / (1 + o % 3))
    ch.subdelay(OUT, 1, 37)
    ch.line(OUT, 1, L0 + 3, -1)
    ch.line(OUT, 2, 5, 2 * L0)
    ch.line(IN, 0, 37, 3 * L0)
    nu = _device(hip, ch, reserve_gain=True)
    nu.set_switch_mode(STAGGERED)
    pc = ch.taps // L0 + 3                                         # the first commit: the history is full
    Fmax = 20000 if name == "big" else 700                          # one run length per schedule: the cache
    periods = pc + (Fmax + Lmax) // L0 + 2 + (ch.taps + Fmax + Lmax) // L0 + 2
    x = _raw(rng, FF[rs], periods * L0, n_in)
    n_f = n_in * n_out
    first = {f: (1, None) for f in range(n_f)}
    first[4] = (1, -0.5)
    second = {f: ((0, None) if f % 2 else (None, (0.0, 2.0, -1.0)[f % 3])) for f in range(0, n_f, 1) if f % 4 != 3}
    R = L0 + max(F // 2, 1)
    state = {"second": None, "seen": []}

    def commit(p, changes):
        assert not nu.switch_busy()
        nu.set_crossfade(F)
        for f, (s, g) in changes.items():
            if s is not None:
                nu.set_coeff(f, s)
            if g is not None:
                nu.set_filter_gain(f, g)
        ch.commit(p, STAGGERED, F, changes)
        state["check"] = p

    def before(p):
        if p == 2:
            nu.set_delay(IN, 0, L0 + 1); ch.set_delay(p, IN, 0, L0 + 1)
            nu.set_subdelay(OUT, 1, -99); ch.set_subdelay(p, OUT, 1, -99)
        if p == pc - 1:
            nu.set_gain_ramp(R); ch.set_gain(p, 0, 0.25, R)
            nu.set_output_gain(0, 0.25)
            nu.set_output_gain(1, 1.5); ch.set_gain(p, 1, 1.5, R)
            nu.set_delay(OUT, 2, L0 + 9); ch.set_delay(p, OUT, 2, L0 + 9)
        if p == pc:
            commit(p, first)
        elif p > pc and state["second"] is None and not nu.switch_busy():
            commit(p, second)
            state["second"] = p
        if p == pc + 2:
            nu.set_mute(OUT, 2, 1); ch.set_mute(p, OUT, 2, 1)
            nu.set_delay(IN, 0, 9); ch.set_delay(p, IN, 0, 9)
        if p == pc + 4:
            nu.set_mute(OUT, 2, 0); ch.set_mute(p, OUT, 2, 0)

    def after(p):
        if state.get("check") == p:
            assert nu.switch_frame() == p * L0
            assert [nu.switch_frame_segment(k) for k in range(len(sched[0]))] == sr.switch_frames(sched, p * L0)
            state["check"] = None

    got, sts = _blocks(nu, x, L0, periods, before, after)
    assert state["second"] is not None and state["second"] <= pc + (F + Lmax) // L0 + 2
    # the ramp did start before the commit and end inside (or right behind) the fade of segment 0
    assert (pc - 1) * L0 + R > pc * L0 and (pc - 1) * L0 + R <= pc * L0 + max(F, 4)
    res = ch.render(x, periods)
    _check("C", got, res, ch, periods, nu, sts)
    assert nu.get_delay(IN, 0) == 9 and nu.get_delay(OUT, 2) == L0 + 9


# ---------------------------------------------------------------- D. sessions

@pytest.mark.parametrize("seed", range(8))
def test_session(hip, seed):
    """one seeded run with every kind of call (nupc_chain_ref.session): bytes or reals, overflow
    structs, status words and the delays in force against the chain model.
    Dithered outputs are 16 or 24 bits wide (nupc_chain_ref.session says why): sessions run up to
    250 000 frames, and the number of rounding ties on a dithered channel grows with the run length
    and with the fineness of a count."""
    s = cr.session(seed)
    rs, sched, half, L0 = s["rs"], s["sched"], s["half"], s["sched"][0][0]
    dt = np.float32 if rs == 4 else np.float64
    ch = cr.Chain(sched, rs, 2, 2, s["infmt"], s["outfmt"], half=half, dither=s["dither"])
    rng = np.random.default_rng(100 + seed)
    for f in range(4):
        ch.add_filter(f % 2, f // 2, _taps(rng, ch.taps, dt, 2), in_scale=0.5 if f % 2 else 1.0,
                      out_scale=-1.0 if f // 2 else 1.0)
    ch.subdelay(IN, 0, 37)
    ch.subdelay(OUT, 1, -25)
    for (io, c), m in s["maxdelay"].items():
        ch.line(io, c, 3, m)
    nu = _device(hip, ch, reserve_gain=True)
    periods = s["periods"]
    x = _raw(rng, s["infmt"], periods * L0, 2)
    evs = {}
    for p, kind, a in s["events"]:
        evs.setdefault(p, []).append((kind, a))
    state = {}

    def before(p):
        for kind, a in evs.get(p, ()):
            if kind == "commit":
                mode, F, changes = a
                assert not nu.switch_busy(), (p, "a switch is still in flight")
                nu.set_switch_mode(mode)
                nu.set_crossfade(F)
                for f, (st, g) in changes.items():
                    if st is not None:
                        nu.set_coeff(f, st)
                    if g is not None:
                        nu.set_filter_gain(f, g)
                ch.commit(p, mode, F, changes)
                state["check"] = (p, mode)
            elif kind == "update":
                f, st, tseed = a
                h = _taps(np.random.default_rng(tseed), ch.taps, dt, 1)[0]
                nu.update_coeff(f, st, h.astype(dt))
                ch.update(f, st, h)
            elif kind == "gain":
                c, g, R = a
                nu.set_gain_ramp(R)
                nu.set_output_gain(c, g)
                ch.set_gain(p, c, g, R)
            elif kind == "delay":
                nu.set_delay(*a)
                ch.set_delay(p, *a)
            elif kind == "mute":
                nu.set_mute(*a)
                ch.set_mute(p, *a)
            elif kind == "subdelay":
                nu.set_subdelay(*a)
                ch.set_subdelay(p, *a)
            elif kind == "reset":
                nu.reset_overflow()
                ch.reset_overflow(p)

    def after(p):
        if state.get("check", (None,))[0] == p:
            mode = state.pop("check")[1]
            t = sr.switch_frames(sched, p * L0)
            if mode == STAGGERED:
                assert nu.switch_frame() == p * L0
                assert [nu.switch_frame_segment(k) for k in range(len(t))] == t
            else:
                assert nu.switch_frame() == cr.aligned_frame(sched, p * L0)

    got, sts = _blocks(nu, x, L0, periods, before, after)
    assert not nu.switch_busy()
    res = ch.render(x, periods)
    _check("D", got, res, ch, periods, nu, sts)
    for io in (IN, OUT):
        assert [nu.get_delay(io, c) for c in range(2)] == ch.cur_delay[io], io
    assert res.overflow[0].n_overflows > 0                          # counted behind the reset
