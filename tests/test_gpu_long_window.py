"""Long-window overlap-save (windows of 4 blocks, coefficient partitions of 3 blocks of taps).

BFHIP_LONG_WINDOW=1 puts small f32 crossbars at L = 8192 on the long plan; each case runs the same
blocks through an engine forced onto the standard plan (BFHIP_LONG_WINDOW=0) and compares, and the
plain case also against the oracle.  Covered: partial last partitions (N = 8, 11, 13), block delays,
coefficient switches with and without cross-fade, in-place partition rewrites, an input-scale change
(the filter moves to a private ring: those blocks run the standard path), both owed-output schedules,
prewarm, run-to-run bit identity, window_blocks() and read_output_spectrum()."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import brutefir_amd as bf  # noqa: E402
import cases  # noqa: E402

pytestmark = pytest.mark.gpu
L = 8192
TOL = 1e-5


def make(monkeypatch, long, N, I, O, delays=None, crossfade=False, overlap=None, n_sets_extra=0):
    monkeypatch.setenv("BFHIP_LONG_WINDOW", "1" if long else "0")
    if overlap is None:
        monkeypatch.delenv("BFHIP_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("BFHIP_OVERLAP", str(overlap))
    e = bf.Engine(L, N, 4, I, O)
    e.set_interleaved(0, "S24_4LE")
    e.set_interleaved(1, "FLOAT_LE")
    for o in range(O):
        for i in range(I):
            h = cases.make_ir(np.random.default_rng(4321 + o * I + i), L * N, I)
            c = e.add_coeff(h)
            e.add_filter(in_ch=[i], out_ch=[o], coeff=c, crossfade=crossfade,
                         delayblocks=0 if delays is None else delays[o][i])
    extra = [e.add_coeff(cases.make_ir(np.random.default_rng(99 + k), L * N, I)) for k in range(n_sets_extra)]
    e.finalize()
    return e, extra


def outs(e, blocks, actions=None):
    res = []
    for k, b in enumerate(blocks):
        if actions and k in actions:
            actions[k](e)
        _, raw = e.block(b)
        res.append(np.frombuffer(raw.tobytes(), np.float32).copy())
    e.sync()
    return res


def compare(a, b, tol=TOL):
    for k, (x, y) in enumerate(zip(a, b)):
        err = cases.rel_rms(x, y)
        assert err <= tol, (k, err)


@pytest.mark.parametrize("N", [8, 11, 13])
def test_long_window_matches_oracle_and_standard(monkeypatch, N):
    import bforacle as bo
    I = O = 8
    g, _ = make(monkeypatch, True, N, I, O)
    assert g.window_blocks == 4 and g.uses_wave_fft
    s, _ = make(monkeypatch, False, N, I, O)
    assert s.window_blocks == 2
    oe, _ = cases.crossbar(bo.Engine, L, N, 4, I, O, "S24_4LE", "FLOAT_LE")
    blocks = cases.raw_blocks(7, N + 3, L, I, "S24_4LE")
    go, so = outs(g, blocks), outs(s, blocks)
    _, oo = cases.run(oe, blocks)
    compare(go, so)
    compare(go, [np.frombuffer(x.tobytes(), np.float32) for x in oo])
    # the same blocks again from a fresh engine: bit-identical
    g2, _ = make(monkeypatch, True, N, I, O)
    assert all(np.array_equal(x, y) for x, y in zip(go, outs(g2, blocks)))
    with pytest.raises(bf.BfhipError):
        g.output_spectrum(0)
    for e in (g, s, g2):
        e.close()


@pytest.mark.parametrize("overlap", [None, 1])
def test_long_window_delays_switches_rewrites_and_fallback(monkeypatch, overlap):
    N, I, O = 11, 8, 16
    rng = np.random.default_rng(5)
    d_in = [int(rng.integers(0, 3)) for _ in range(I)]        # per input: every (ring, delay) entry stays a full crossbar row
    delays = [list(d_in) for _ in range(O)]
    new_taps = cases.make_ir(np.random.default_rng(77), L, I)
    engines = []
    for long in (True, False):
        e, extra = make(monkeypatch, long, N, I, O, delays=delays, crossfade=True, overlap=overlap, n_sets_extra=2)
        engines.append((e, extra))
    (g, gx), (s, sx) = engines
    assert g.window_blocks == 4 and s.window_blocks == 2
    if overlap == 1:
        assert g.block_mode == 3
    actions = {
        N + 2: lambda e: e.set_coeff(3, e_extra(e)[0]),                 # cross-fade block, then long again
        N + 4: lambda e: e.update_coeff_block(5, 4, new_taps),          # one partition of a set in use
        N + 6: lambda e: e.set_scale(9, 0, 0, 0.5),                      # private ring: standard blocks
    }
    extras = {id(g): gx, id(s): sx}

    def e_extra(e):
        return extras[id(e)]
    blocks = cases.raw_blocks(11, N + 10, L, I, "S24_4LE")
    compare(outs(g, blocks, actions), outs(s, blocks, actions))
    g.close()
    s.close()


def test_long_window_prewarm(monkeypatch):
    N, I, O = 8, 8, 8
    g, _ = make(monkeypatch, True, N, I, O)
    s, _ = make(monkeypatch, False, N, I, O)
    g.prewarm()
    s.prewarm()
    blocks = cases.raw_blocks(3, 4, L, I, "S24_4LE")
    compare(outs(g, blocks), outs(s, blocks))
    g.close()
    s.close()


def test_long_window_gate(monkeypatch):
    """unset: the size threshold decides (below 1 GiB of coefficients: the standard plan)"""
    monkeypatch.delenv("BFHIP_LONG_WINDOW", raising=False)
    e, _ = cases.crossbar(bf.Engine, L, 8, 4, 8, 8, "S24_4LE", "S24_4LE")
    assert e.window_blocks == 2
    e.close()
    f, _ = cases.crossbar(bf.Engine, L, 8, 8, 4, 4, "S24_4LE", "S24_4LE")
    assert f.window_blocks == 2
    f.close()


def _bench_shape(I, O, N, rs, diagonal=False):
    """a bench.py workload's engine: I x O crossbar (or I one-to-one filters), device taps"""
    import torch
    e = bf.Engine(L, N, rs, I, O)
    fmt = "S24_4LE" if rs == 4 else "FLOAT64_LE"
    e.set_interleaved(0, fmt)
    e.set_interleaved(1, fmt)
    pairs = [(o, o) for o in range(O)] if diagonal else [(o, i) for o in range(O) for i in range(I)]
    e.reserve_coeffs(float(len(pairs)) * N * 2 * L * rs)
    h = torch.randn(L * N, device="cuda", dtype=torch.float32 if rs == 4 else torch.float64) * 1e-4
    for o, i in pairs:
        e.add_filter(in_ch=[i], out_ch=[o], coeff=e.add_coeff_dev(h, L * N))
    torch.cuda.synchronize()
    e.finalize()
    return e


@pytest.mark.parametrize("name,shape,want", [
    ("C", (64, 64, 32, 4, False), 4),
    ("B", (8, 8, 8, 4, False), 2),
    ("D", (256, 256, 16, 4, True), 2),          # one-to-one, 256 MiB of coefficients
    ("E", (2, 2, 128, 8, False), 2),            # float64
    ("F", (32, 32, 32, 8, False), 2),           # float64, 4 GiB
])
def test_bench_shapes_select_the_window(monkeypatch, name, shape, want):
    """config C's shape takes the long plan by default; B, D, E and F do not"""
    monkeypatch.delenv("BFHIP_LONG_WINDOW", raising=False)
    e = _bench_shape(*shape)
    assert e.window_blocks == want, name
    if name == "C":
        assert e.uses_wave_fft and e.uses_stream_layout
    e.close()


def test_phase_calls_run_the_standard_plan(monkeypatch):
    """an engine driven through the phase calls hands standard spectra to its caller: from its first
    phase call on it runs the standard plan, with the same results as an engine that never had one"""
    import torch
    N, I, O = 8, 8, 8
    outs_ = []
    for long in (True, False):
        e, _ = make(monkeypatch, long, N, I, O)
        z = torch.zeros(O, L, 2, dtype=torch.float32, device="cuda")
        raw_out = torch.zeros(L * O, dtype=torch.float32, device="cuda")
        got = []
        for b in cases.raw_blocks(9, N + 2, L, I, "S24_4LE"):
            e.inputs_dev(torch.from_numpy(b.view(np.int32).copy()).cuda())
            e.mac_dev(z)
            e.advance()
            e.outputs_dev(z, 0, O, raw_out)
            torch.cuda.synchronize()
            got.append(raw_out.cpu().numpy().copy())
        assert e.window_blocks == 2
        outs_.append(got)
        e.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs_))


@pytest.mark.parametrize("split", ["groups", "interleaved"])
def test_shards_on_the_long_plan_write_what_the_whole_engine_writes(monkeypatch, split):
    """the host's filter processes (one shard engine each, foreign terms taken out of the entries)
    take the long plan exactly when the one-process engine does, and the outputs they leave in the
    shared buffer are bit for bit the one-process engine's (24-bit: the rounding must match too)"""
    monkeypatch.setenv("BFHIP_LONG_WINDOW", "1")
    monkeypatch.delenv("BFHIP_OVERLAP", raising=False)
    N, I, O = 11, 8, 16
    owner = [(o // 8) % 2 if split == "groups" else o % 2 for o in range(O)]

    def build(k):
        e = bf.Engine(L, N, 4, I, O)
        e.set_interleaved(0, "S24_4LE")
        e.set_interleaved(1, "S24_4LE")
        for o in range(O):
            for i in range(I):
                c = e.add_coeff(cases.make_ir(np.random.default_rng(4321 + o * I + i), L * N, I))
                e.add_filter(in_ch=[i], out_ch=[o], coeff=c)
        if k is not None:
            for fi in range(O * I):
                e.set_filter_active(fi, owner[fi // I] == k)
            for o in range(O):
                e.set_output_active(o, owner[o] == k)
        e.finalize()
        return e
    whole = build(None)
    shards = [build(k) for k in range(2)]
    assert [whole.window_blocks] + [s.window_blocks for s in shards] == [4, 4, 4]
    for b, blk in enumerate(cases.raw_blocks(13, N + 4, L, I, "S24_4LE", amplitude=0.6)):
        _, w = whole.block(blk)
        shared = np.full(w.size, 0xA5, np.uint8)
        for s in shards:
            s.block(blk, out=shared)
        assert np.array_equal(shared, w), b
    for e in [whole] + shards:
        e.close()
