"""Two-tier look-ahead long-window MAC (kernels.h: mac_la_kernel<float, 7> / <float, 6>, la_far_phase): a
call reads partition 0 for its own block, p = 1 of one third of the entries for the next three blocks and
p >= 2 of one sixth of the entries for the next six.

BFHIP_LONG_WINDOW=1, BFHIP_LOOKAHEAD=1 and BFHIP_LOOKAHEAD_FAR=1 put small f32 crossbars at L = 8192 on
it (the gate needs L = 8192).  8 x 8: far slices of 2/2/1/1/1/1 entries; 3 x 8: 1/1/1/0/0/0, three empty
slices.  Every case runs the same blocks through an engine on the standard plan (the plain cases also on
the single-tier look-ahead plan, N = 11 also through the oracle) and compares at the project's 1e-5
relative RMS.  Covered: partial and whole last partitions (N = 9, 11, 13, 20), the gates (N = 8; no
BFHIP_LOOKAHEAD_FAR), block delays, a coefficient switch with cross-fade, an in-place partition rewrite
and a scale change at each value of t mod 6 under both owed-output schedules with the launch counts,
prewarm, run-to-run bit identity, independence of the phase t mod 6, element 0."""
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


def make(monkeypatch, plan, N, I, O, delays=None, crossfade=False, overlap=None, n_sets_extra=0, far_env="1"):
    """plan: "far" (long windows, look-ahead, far tier), "la" (single-tier look-ahead), "std".  far_env:
    what BFHIP_LOOKAHEAD_FAR is on the "far" plan (None: unset).  The standard plan would cut the few
    entries of such a group along p to get its workgroups (at N = 20 also with eight of them), and the long
    plan takes whole entries only: every engine is held to one chunk per entry"""
    monkeypatch.setenv("BFHIP_MAC_TARGET_WGS", str(16 * ((O + 7) // 8) * I))
    monkeypatch.setenv("BFHIP_LONG_WINDOW", "0" if plan == "std" else "1")
    monkeypatch.setenv("BFHIP_LOOKAHEAD", "0" if plan == "std" else "1")
    if plan == "far" and far_env is None:
        monkeypatch.delenv("BFHIP_LOOKAHEAD_FAR", raising=False)
    else:
        monkeypatch.setenv("BFHIP_LOOKAHEAD_FAR", far_env if plan == "far" else "0")
    if overlap is None:
        monkeypatch.delenv("BFHIP_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("BFHIP_OVERLAP", str(overlap))
    e = bf.Engine(L, N, 4, I, O)
    e.set_interleaved(0, "S24_4LE")
    e.set_interleaved(1, "FLOAT_LE")
    for o in range(O):
        for i in range(I):
            c = e.add_coeff(ir(4321 + o * I + i, L * N, I))
            e.add_filter(in_ch=[i], out_ch=[o], coeff=c, crossfade=crossfade,
                         delayblocks=0 if delays is None else delays[i])
    extra = [e.add_coeff(ir(99 + k, L * N, I)) for k in range(n_sets_extra)]
    e.finalize()
    return e, extra


def outs(e, blocks, actions=None, each=None):
    res = []
    for k, b in enumerate(blocks):
        if actions and k in actions:
            actions[k](e)
        _, raw = e.block(b)
        res.append(np.frombuffer(raw.tobytes(), np.float32).copy())
        if each:
            each(e, k)
    e.sync()
    return res


def compare(a, b, tol=TOL):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        err = cases.rel_rms(x, y)
        assert err <= tol, (k, err)


@pytest.mark.parametrize("N", [9, 11, 13, 20])
@pytest.mark.parametrize("I,O", [(8, 8), (3, 8)])
def test_far_matches_single_tier_standard_and_oracle(monkeypatch, N, I, O):
    """N + 12 blocks: the start (the far buffers of the first six blocks are zeros: no far partition reaches
    a block that exists), warm-up with the partitions of the six blocks ahead differing, steady state"""
    g, _ = make(monkeypatch, "far", N, I, O)
    assert g.lookahead_far_blocks == 6 and g.lookahead_blocks == 3 and g.window_blocks == 4
    blocks = cases.raw_blocks(7, N + 12, L, I, "S24_4LE")
    counts = []
    go = outs(g, blocks, each=lambda e, k: counts.append(e.mac_counts))
    g.close()
    # the head pass (one launch) in every block but at most the first six, the full long MAC (two) in those
    n_launch, n_head, n_full = counts[-1]
    assert n_head + n_full == len(blocks) and n_full <= 6 and n_launch == n_head + 2 * n_full
    assert [b[0] - a[0] for a, b in zip(counts[6:], counts[7:])] == [1] * (len(blocks) - 7)
    g2, _ = make(monkeypatch, "far", N, I, O)
    assert all(np.array_equal(x, y) for x, y in zip(go, outs(g2, blocks)))      # run to run: the same bits
    g2.close()
    for plan in ("la", "std"):
        s, _ = make(monkeypatch, plan, N, I, O)
        assert s.lookahead_far_blocks == 0 and s.lookahead_blocks == (3 if plan == "la" else 0)
        compare(go, outs(s, blocks))
        s.close()
    if N == 11:
        import bforacle as bo
        oe, _ = cases.crossbar(bo.Engine, L, N, 4, I, O, "S24_4LE", "FLOAT_LE")
        _, oo = cases.run(oe, blocks)
        compare(go, [np.frombuffer(x.tobytes(), np.float32) for x in oo])


def test_far_gates(monkeypatch):
    I, O = 8, 8
    # N = 8: three long partitions, the last one (p = 2) shifted by one block reads block t - 5 -- which
    # a call six blocks earlier does not have.  The variable set: one tier, and that engine's bits
    blocks = cases.raw_blocks(5, 8 + 8, L, I, "S24_4LE")
    g, _ = make(monkeypatch, "far", 8, I, O)
    assert g.lookahead_far_blocks == 0 and g.lookahead_blocks == 3
    go = outs(g, blocks)
    g.close()
    s, _ = make(monkeypatch, "la", 8, I, O)
    assert s.lookahead_far_blocks == 0 and s.lookahead_blocks == 3
    so = outs(s, blocks)
    s.close()
    assert all(np.array_equal(x, y) for x, y in zip(go, so))
    # BFHIP_LOOKAHEAD=1 alone does not switch the far tier on below 1 GiB of coefficients
    e, _ = make(monkeypatch, "far", 11, I, O, far_env=None)
    assert e.lookahead_far_blocks == 0 and e.lookahead_blocks == 3
    e.close()


def test_far_block_delays(monkeypatch):
    N, I, O = 11, 8, 8
    delays = [0, 1, 2, 0, 1, 2, 2, 0]
    blocks = cases.raw_blocks(13, N + 12, L, I, "S24_4LE")
    res = []
    for plan in ("far", "std"):
        e, _ = make(monkeypatch, plan, N, I, O, delays=delays)
        assert e.lookahead_far_blocks == (6 if plan == "far" else 0)
        res.append(outs(e, blocks))
        e.close()
    compare(res[0], res[1])


def _event(kind, new_taps):
    if kind == "set_coeff":
        return lambda e, extra: e.set_coeff(3, extra[0])                 # a cross-fade block, then long again
    if kind == "update_coeff_block":
        return lambda e, extra: e.update_coeff_block(5, 4, new_taps)     # one partition of a set in use
    return lambda e, extra: e.set_scale(9, 0, 0, 0.5)                    # private ring: standard blocks from here on


@pytest.mark.parametrize("phase", range(6))
@pytest.mark.parametrize("overlap", [None, 1])
@pytest.mark.parametrize("kind", ["set_coeff", "update_coeff_block", "set_scale"])
def test_far_events_at_every_phase(monkeypatch, kind, overlap, phase):
    """what is stored ahead when a set is switched, rewritten or rescaled must not reach an output: the
    event at six consecutive blocks (each value of t mod 6), per-input delays 0 - 2.  After it the full
    long MAC runs (two launches a block) until six far passes have refilled a block's buffers, then the
    head pass is back with one launch per block"""
    N, I, O = 11, 8, 8
    delays = [int(v) for v in np.random.default_rng(5).integers(0, 3, I)]
    new_taps = ir(77, L, I)
    at = N + 1 + phase
    blocks = cases.raw_blocks(11, at + 11, L, I, "S24_4LE")
    act = _event(kind, new_taps)
    res, counts = {}, []
    for plan in ("far", "std"):
        e, extra = make(monkeypatch, plan, N, I, O, delays=delays, crossfade=True, overlap=overlap, n_sets_extra=1)
        assert e.lookahead_far_blocks == (6 if plan == "far" else 0)
        if overlap == 1:
            assert e.block_mode == 3
        res[plan] = outs(e, blocks, {at: lambda eng, x=extra: act(eng, x)},
                         each=(lambda eng, k: counts.append(eng.mac_counts)) if plan == "far" else None)
        e.close()
    compare(res["far"], res["std"])
    print(kind, overlap, phase, "(launches, head blocks, full blocks) per block:", counts)
    launches, heads, fulls = ([c[i] for c in counts] for i in range(3))
    # up to the event: the head pass, or (at the start, at most six times) the full long MAC
    f0 = fulls[at - 1]
    assert heads[at - 1] + f0 == at and f0 <= 6 and launches[at - 1] == heads[at - 1] + 2 * f0
    if kind == "set_scale":
        assert heads[-1] == heads[at - 1] and fulls[-1] == f0         # standard blocks from the event on
        return
    back = next(k for k in range(at, len(counts)) if heads[k] > heads[at - 1])
    assert 6 <= back - at <= 7                                 # (the cross-fade block itself runs the standard MAC)
    assert fulls[back - 1] == f0 + 6 and fulls[-1] == f0 + 6   # six full long MACs, none once the head pass is back
    assert launches[back - 1] - launches[at - 1] == 2 * 6 + (back - at - 6)
    n_back = len(counts) - back
    assert n_back >= 3
    assert [heads[k] - heads[k - 1] for k in range(back, len(counts))] == [1] * n_back
    assert [launches[k] - launches[k - 1] for k in range(back, len(counts))] == [1] * n_back


def test_far_prewarm(monkeypatch):
    N, I, O = 11, 8, 8
    blocks = cases.raw_blocks(3, 9, L, I, "S24_4LE")
    res = []
    for plan in ("far", "std"):
        e, _ = make(monkeypatch, plan, N, I, O)
        e.prewarm()
        res.append(outs(e, blocks))
        e.close()
    compare(res[0], res[1])


def test_far_result_does_not_depend_on_the_phase(monkeypatch):
    """engine B gets s = 1 .. 5 leading silent blocks that engine A does not: every later block then runs
    at another value of t mod 6 (and of t mod 3).  Added zeros are exact, so B's outputs, s blocks later,
    are A's bits"""
    N, I, O = 11, 8, 8
    blocks = cases.raw_blocks(21, 14, L, I, "S24_4LE")
    a, _ = make(monkeypatch, "far", N, I, O)
    a.prewarm()
    ao = outs(a, blocks)
    a.close()
    for s in range(1, 6):
        b, _ = make(monkeypatch, "far", N, I, O)
        b.prewarm()
        bo_ = outs(b, [np.zeros_like(blocks[0])] * s + blocks)
        b.close()
        assert not any(np.any(x) for x in bo_[:s])
        for k, (x, y) in enumerate(zip(ao, bo_[s:])):
            assert np.array_equal(x, y), (s, k)


def _tone_blocks(kind, n_blocks, I):
    """S24_4LE blocks of a constant (its spectrum is DC only) or of +c, -c, +c ... (Nyquist only)"""
    c = int(0.1 * (1 << 23))
    col = np.full(L, c, np.int32)
    if kind == "nyquist":
        col[1::2] = -c
    return [np.ascontiguousarray(np.repeat(col[:, None], I, axis=1)) for _ in range(n_blocks)]


@pytest.mark.parametrize("kind", ["dc", "nyquist"])
def test_far_element_0(monkeypatch, kind):
    """a constant input excites DC alone, the alternating one Nyquist alone: both live in element 0 of the
    packed spectrum, the one product with a fix-up, and the output is nothing but that product"""
    N, I, O = 11, 8, 8
    blocks = _tone_blocks(kind, N + 8, I)
    res = {}
    for plan in ("far", "std"):
        e, _ = make(monkeypatch, plan, N, I, O)
        assert e.lookahead_far_blocks == (6 if plan == "far" else 0)
        res[plan] = outs(e, blocks)
        e.close()
    for k, (a, b) in enumerate(zip(res["far"], res["std"])):
        assert np.any(b), k
        assert cases.rel_rms(a, b) <= TOL, (k, cases.rel_rms(a, b))
