"""Look-ahead long-window MAC (kernels.h: mac_la_head_kernel, mac_la_tail_kernel): a call reads one
third of the tail partitions once for the next three blocks, and partition 0 for its own.

BFHIP_LONG_WINDOW=1 and BFHIP_LOOKAHEAD=1 put small f32 crossbars at L = 8192 on it; every case runs
the same blocks through an engine on the standard plan (and the plain cases also through the long plan
without look-ahead, and the oracle) and compares at the project's 1e-5 relative RMS.  Covered: slices
of 3/3/2 and 1/1/0 entries, partial last partitions (N = 8, 11, 13), block delays, a coefficient switch
with cross-fade, an in-place partition rewrite and a scale change at each value of t mod 3, both
owed-output schedules, prewarm, run-to-run bit identity, independence of the phase t mod 3, the gates."""
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

_irs = {}


def ir(seed, taps, I):
    key = (seed, taps, I)
    if key not in _irs:
        _irs[key] = cases.make_ir(np.random.default_rng(seed), taps, I)
    return _irs[key]


def make(monkeypatch, plan, N, I, O, delays=None, crossfade=False, overlap=None, n_sets_extra=0, taps=None):
    """plan: "la" (long windows + look-ahead), "long" (long windows only), "std".  With two entries per
    group the standard plan would cut its entries along p to get its workgroups (13 partitions: three
    chunks), and the long plan takes whole entries only: such engines are held to one chunk per entry"""
    if I < 3:
        monkeypatch.setenv("BFHIP_MAC_TARGET_WGS", str(16 * ((O + 7) // 8) * I))
    else:
        monkeypatch.delenv("BFHIP_MAC_TARGET_WGS", raising=False)
    monkeypatch.setenv("BFHIP_LONG_WINDOW", "0" if plan == "std" else "1")
    monkeypatch.setenv("BFHIP_LOOKAHEAD", "1" if plan == "la" else "0")
    if overlap is None:
        monkeypatch.delenv("BFHIP_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("BFHIP_OVERLAP", str(overlap))
    e = bf.Engine(L, N, 4, I, O)
    e.set_interleaved(0, "S24_4LE")
    e.set_interleaved(1, "FLOAT_LE")
    for o in range(O):
        for i in range(I):
            c = e.add_coeff(ir(4321 + o * I + i, L * N if taps is None else taps, I))
            e.add_filter(in_ch=[i], out_ch=[o], coeff=c, crossfade=crossfade,
                         delayblocks=0 if delays is None else delays[i])
    extra = [e.add_coeff(ir(99 + k, L * N, I)) for k in range(n_sets_extra)]
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


def compare(a, b, tol=TOL, first=0):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        err = cases.rel_rms(x, y)
        assert k < first or err <= tol, (k, err)


@pytest.mark.parametrize("N", [8, 11, 13])
@pytest.mark.parametrize("I,O", [(8, 8), (2, 8)])
def test_lookahead_matches_long_standard_and_oracle(monkeypatch, N, I, O):
    """I = 8: slices of 3, 3 and 2 entries; I = 2: one empty slice.  N + 6 blocks: the start (the ahead
    buffers of the first three blocks are zeros: no tail reaches a block that exists), warm-up with the
    partitions of the three blocks ahead differing, steady state"""
    import bforacle as bo
    g, _ = make(monkeypatch, "la", N, I, O)
    assert g.lookahead_blocks == 3 and g.window_blocks == 4
    blocks = cases.raw_blocks(7, N + 6, L, I, "S24_4LE")
    go = outs(g, blocks)
    g.close()
    g2, _ = make(monkeypatch, "la", N, I, O)
    assert all(np.array_equal(x, y) for x, y in zip(go, outs(g2, blocks)))      # run to run: the same bits
    g2.close()
    for plan in ("long", "std"):
        s, _ = make(monkeypatch, plan, N, I, O)
        assert s.lookahead_blocks == 0 and s.window_blocks == (4 if plan == "long" else 2)
        compare(go, outs(s, blocks))
        s.close()
    oe, _ = cases.crossbar(bo.Engine, L, N, 4, I, O, "S24_4LE", "FLOAT_LE")
    _, oo = cases.run(oe, blocks)
    compare(go, [np.frombuffer(x.tobytes(), np.float32) for x in oo])


def _event(kind, new_taps):
    if kind == "set_coeff":
        return lambda e, extra: e.set_coeff(3, extra[0])                 # a cross-fade block, then long again
    if kind == "update_coeff_block":
        return lambda e, extra: e.update_coeff_block(5, 4, new_taps)     # one partition of a set in use
    return lambda e, extra: e.set_scale(9, 0, 0, 0.5)                    # private ring: standard blocks from here on


@pytest.mark.parametrize("overlap", [None, 1])
@pytest.mark.parametrize("kind", ["set_coeff", "update_coeff_block", "set_scale"])
def test_lookahead_events_at_every_phase(monkeypatch, kind, overlap):
    """what is stored ahead when a set is switched, rewritten or rescaled must not reach an output:
    the event at three consecutive blocks (each value of t mod 3), per-input delays 0 - 2"""
    N, I, O = 11, 8, 8
    delays = [int(v) for v in np.random.default_rng(5).integers(0, 3, I)]
    new_taps = ir(77, L, I)
    blocks = cases.raw_blocks(11, N + 9, L, I, "S24_4LE")
    act = _event(kind, new_taps)
    for phase in range(3):
        res = []
        for plan in ("la", "std"):
            e, extra = make(monkeypatch, plan, N, I, O, delays=delays, crossfade=True, overlap=overlap, n_sets_extra=1)
            assert e.lookahead_blocks == (3 if plan == "la" else 0)
            if overlap == 1:
                assert e.block_mode == 3
            res.append(outs(e, blocks, {N + 1 + phase: lambda eng, x=extra: act(eng, x)}))
            e.close()
        compare(res[0], res[1])


def test_lookahead_prewarm(monkeypatch):
    N, I, O = 8, 8, 8
    blocks = cases.raw_blocks(3, 4, L, I, "S24_4LE")
    res = []
    for plan in ("la", "std"):
        e, _ = make(monkeypatch, plan, N, I, O)
        e.prewarm()
        res.append(outs(e, blocks))
        e.close()
    compare(res[0], res[1])


def test_lookahead_result_does_not_depend_on_the_phase(monkeypatch):
    """engine B gets one leading silent block that engine A does not: every later block then runs at the
    next value of t mod 3.  Added zeros are exact, so B's outputs, one block later, are A's bits"""
    N, I, O = 11, 8, 8
    blocks = cases.raw_blocks(21, 8, L, I, "S24_4LE")
    a, _ = make(monkeypatch, "la", N, I, O)
    a.prewarm()
    ao = outs(a, blocks)
    a.close()
    b, _ = make(monkeypatch, "la", N, I, O)
    b.prewarm()
    bo_ = outs(b, [np.zeros_like(blocks[0])] + blocks)
    b.close()
    assert not np.any(bo_[0])
    for k, (x, y) in enumerate(zip(ao, bo_[1:])):
        assert np.array_equal(x, y), k


def test_lookahead_gates(monkeypatch):
    N, I, O = 8, 8, 8
    # long windows alone do not switch it on below 1 GiB of coefficients
    monkeypatch.setenv("BFHIP_LONG_WINDOW", "1")
    monkeypatch.delenv("BFHIP_LOOKAHEAD", raising=False)
    e, _ = cases.crossbar(bf.Engine, L, N, 4, I, O, "S24_4LE", "FLOAT_LE")
    assert e.window_blocks == 4 and e.lookahead_blocks == 0
    e.close()
    # a filter of 4 partitions: the last long partition is p = 1, shifted by two blocks -- it reads
    # block t - 1, which a call three blocks earlier does not have
    blocks = cases.raw_blocks(5, N + 3, L, I, "S24_4LE")
    g, _ = make(monkeypatch, "la", N, I, O, taps=4 * L)
    assert g.lookahead_blocks == 0
    s, _ = make(monkeypatch, "std", N, I, O, taps=4 * L)
    compare(outs(g, blocks), outs(s, blocks))
    g.close()
    s.close()


def test_lookahead_gate_shards_and_phase_calls(monkeypatch):
    import torch
    N, I, O = 8, 8, 16
    monkeypatch.setenv("BFHIP_LONG_WINDOW", "1")
    monkeypatch.setenv("BFHIP_LOOKAHEAD", "1")
    monkeypatch.delenv("BFHIP_OVERLAP", raising=False)
    e = bf.Engine(L, N, 4, I, O)
    e.set_interleaved(0, "S24_4LE")
    e.set_interleaved(1, "S24_4LE")
    for o in range(O):
        for i in range(I):
            e.add_filter(in_ch=[i], out_ch=[o], coeff=e.add_coeff(ir(4321 + o * I + i, L * N, I)))
    for fi in range(O * I):
        e.set_filter_active(fi, fi // I < 8)
    for o in range(O):
        e.set_output_active(o, o < 8)
    e.finalize()
    assert e.window_blocks == 4 and e.lookahead_blocks == 0           # a shard
    e.close()
    p, _ = make(monkeypatch, "la", N, 8, 8)
    assert p.lookahead_blocks == 3
    z = torch.zeros(8, L, 2, dtype=torch.float32, device="cuda")
    p.inputs_dev(torch.from_numpy(cases.raw_blocks(9, 1, L, 8, "S24_4LE")[0].view(np.int32).copy()).cuda())
    p.mac_dev(z)
    torch.cuda.synchronize()
    assert p.lookahead_blocks == 0 and p.window_blocks == 2           # driven through the phase calls
    p.close()
