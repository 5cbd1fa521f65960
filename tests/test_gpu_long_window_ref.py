"""The long-window plan (4-block windows, 3-block partitions, kernels.h) held to the float64 crossbar
model (tests/xbar_ref.py), next to the standard plan run on the same blocks.

Every case builds two engines the same way, BFHIP_LONG_WINDOW=1 and =0, drives them with the same
blocks and control calls, and holds both to the model: float outputs within 2e-5 relative RMS on
every block and 1e-5 over the run; S16 outputs exact except within 0.05 LSB of a rounding threshold
(there within one count), 24- and 32-bit outputs within 2e-6 of full scale, overflow counts exact.  The long engine's
window_blocks() is asserted on every block where the case expects a plan (4: long; 2: the plan falls
back), so that no case passes by quietly running the standard plan.  Every (output, input) pair has
its own impulse response.

Run-time delay changes: the engine gives a filter whose delay (or input scale) changes a private
ring, with the reference's history semantics (bfrun.c:1600-1641, promote_filter); such a filter is
no longer part of a plain crossbar, so the long plan falls back from that block on.  The cases pin
exactly that, and the model follows the reference's ring slots through the change."""
import ctypes as C
import mmap
import os

import numpy as np
import pytest

import brutefir_amd as bf
import cases
import xbar_ref as xr

from long_rig import L, TOL_BLOCK, TOL_RUN, Rig, _ir, blocks_for, both, drive, hold  # noqa: F401

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ a. shapes

@pytest.mark.parametrize("N", [8, 9, 10, 11, 12, 13])
def test_shapes_partition_counts(monkeypatch, N):
    rig = Rig(N, 8, 8, seed=100 * N)
    both(monkeypatch, rig, blocks_for(rig, N + 3))


def test_shape_many_partitions(monkeypatch):
    """N = 32: 11 long partitions, the last one end-aligned (shift 1), a long start-up.  On 16 x 16:
    an 8 x 8 crossbar with N >= 16 gets a MAC plan the long layout does not take"""
    N = 32
    rig = Rig(N, 16, 16, seed=3200)
    both(monkeypatch, rig, blocks_for(rig, N + 3))


@pytest.mark.parametrize("I,O,want", [(5, 16, 4), (12, 16, 4), (8, 12, 2)])
def test_shapes_channel_counts(monkeypatch, I, O, want):
    """inputs not a multiple of 8 stay long (xcd_channel over the long K1); an output count that is
    not a multiple of 8 (a masked last group) falls back, and stays right"""
    rig = Rig(11, I, O, seed=3 + I * O)
    both(monkeypatch, rig, blocks_for(rig, 14), win=lambda k: want)


# ------------------------------------------------------------------ b. lengths

def test_all_sets_two_blocks_short(monkeypatch):
    N = 11
    rig = Rig(N, 8, 8, seed=21, lengths={(o, i): (N - 2) * L for o in range(8) for i in range(8)})
    both(monkeypatch, rig, blocks_for(rig, N + 3))


def test_one_short_set_falls_back(monkeypatch):
    """an entry with one short term is no longer dense: the plan falls back, outputs stay right"""
    N = 11
    rig = Rig(N, 8, 8, seed=22, lengths={(3, 5): 4 * L + 100})
    both(monkeypatch, rig, blocks_for(rig, N + 3), win=lambda k: 2)


# ------------------------------------------------------------------ c. delays

@pytest.mark.parametrize("N", [8, 11, 12])
def test_column_delays_up_to_clamped(monkeypatch, N):
    """per-input delays N - 3, N - 2, N - 1 and N + 4 (clamped to N - 1): q_end = 3, 2, 1 -- the last
    long partition starts below block 0 of the filter"""
    d = {0: N - 3, 1: N - 2, 2: N - 1, 3: N + 4, 4: 0, 5: 1, 6: 2, 7: 5}
    rig = Rig(N, 8, 8, seed=31 + N, delays=d)
    both(monkeypatch, rig, blocks_for(rig, 2 * N + 2))


@pytest.mark.parametrize("whole_column", [True, False])
def test_runtime_delay_change(monkeypatch, whole_column):
    """set_delayblocks at run time gives the filters their own rings (the reference's history
    semantics): the long plan falls back from that block on, and both plans follow the model through
    the N blocks in which the rings hold blocks of both delays"""
    N, I, O = 11, 8, 8
    rig = Rig(N, I, O, seed=41, delays={2: 1})
    t = N + 2
    fs = [o * I + 2 for o in range(O)] if whole_column else [3 * I + 2]
    actions = {t: [("delay", f, 4) for f in fs]}
    both(monkeypatch, rig, blocks_for(rig, t + N + 3), actions, win=lambda k: 4 if k < t else 2)


# ------------------------------------------------------------------ d. in-place rewrites

@pytest.mark.parametrize("N", [11, 12])
def test_rewrite_every_partition(monkeypatch, N):
    """update_coeff_block on every standard partition of a set in use, one per period: each long
    partition, the end-aligned last one and the block before it included"""
    I = O = 8
    rig = Rig(N, I, O, seed=51 + N)
    rng = np.random.default_rng(N)
    t0 = 3
    actions = {t0 + b: [("rewrite", (3, 5), b, _ir(int(rng.integers(1 << 30)), L, I))] for b in range(N)}
    both(monkeypatch, rig, blocks_for(rig, t0 + N + 2), actions)


def test_rewrites_beyond_the_cut_and_together(monkeypatch):
    """a rewrite at or beyond q_end of a delayed filter (changes nothing), two rewrites in one period,
    a rewrite in the period of another filter's set_coeff"""
    N, I, O = 11, 8, 8
    rig = Rig(N, I, O, seed=61, delays={6: 3}, n_extra=1)       # input 6: q_end = 8
    rng = np.random.default_rng(6)
    new = lambda: _ir(int(rng.integers(1 << 30)), L, I)         # noqa: E731
    t = N + 1
    actions = {t: [("rewrite", (1, 6), 8, new()), ("rewrite", (1, 6), 10, new())],
               t + 1: [("rewrite", (2, 0), 9, new()), ("rewrite", (4, 4), 1, new())],
               t + 2: [("coeff", 5 * I + 1, ("x", 0)), ("rewrite", (6, 7), 10, new())],
               t + 3: [("rewrite", (1, 6), 7, new())]}
    both(monkeypatch, rig, blocks_for(rig, t + 6), actions)


def test_rewrite_around_a_crossfade_block(monkeypatch):
    """the cross-fade block runs the standard path on the long engine: a rewrite issued in that
    period (after the set_coeff) and one issued right after the fade block (no long plan in force)
    must reach the long partitions when the plan comes back on the next block"""
    N, I, O = 11, 8, 8
    rig = Rig(N, I, O, seed=71, n_extra=1, crossfade=True)
    rng = np.random.default_rng(7)
    t = N + 2
    actions = {t: [("coeff", 2 * I + 3, ("x", 0)), ("rewrite", (0, 1), 9, _ir(int(rng.integers(1 << 30)), L, I))],
               t + 1: [("rewrite", (5, 5), 10, _ir(int(rng.integers(1 << 30)), L, I)),
                       ("rewrite", (6, 2), 4, _ir(int(rng.integers(1 << 30)), L, I))]}
    both(monkeypatch, rig, blocks_for(rig, t + 5), actions, win=lambda k: 2 if k == t else 4)


# ------------------------------------------------------------------ e. watched sets

def _cv():
    lib = bf.lib()
    lib.convolver_coeffs2cbuf.restype = C.c_void_p
    lib.convolver_coeffs2cbuf.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
    lib.convolver_runtime_coeffs2cbuf.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.convolver_init(None, L, 4) == 1
    return lib


@pytest.mark.parametrize("lazy", [False, True])
def test_watched_set_rewritten_by_another_process(monkeypatch, lazy):
    """a set in shared memory, rewritten by a forked child (no GPU state touched there) in a middle
    long partition and in the last one; lazy: the set is registered lazily and a filter switches to it"""
    N, I, O = 11, 8, 8
    cv = _cv()
    rig = Rig(N, I, O, seed=81, n_extra=1)
    key = ("x", 0) if lazy else (0, 0)
    h = rig.sets[key].astype(np.float32)
    shm = mmap.mmap(-1, N * 2 * L * 4)
    base = np.frombuffer(shm, np.float32)
    addr = [base[b * 2 * L:].ctypes.data for b in range(N)]

    def render():
        for b in range(N):
            t = np.ascontiguousarray(h[b * L:(b + 1) * L])
            assert cv.convolver_coeffs2cbuf(t.ctypes.data_as(C.c_void_p), L, 1.0, C.c_void_p(addr[b])) == addr[b]

    def hook(e):
        e.cid[key] = e.add_coeff_processed_blocks(addr, watch=True, lazy=lazy)

    engines = []
    for long in (True, False):
        render()
        engines.append(rig.engine(monkeypatch, long, sets_hook=hook))
    if lazy:
        assert not engines[0].coeff_is_resident(engines[0].cid[key])
    rng = np.random.default_rng(8)
    sw = 2 if lazy else None
    fsw = 4 * I + 4
    rw = {N + 1: 4, N + 3: 9}                # long partition 1; the last one (standard 8..10)
    parts = {t: _ir(int(rng.integers(1 << 30)), L, I).astype(np.float32) for t in rw}
    blocks = blocks_for(rig, N + 6)
    outs = [[] for _ in engines]
    for k, blk in enumerate(blocks):
        if k == sw:
            for e in engines:
                e.set_coeff(fsw, e.cid[key])
        if k in rw:
            pid = os.fork()
            if pid == 0:
                try:
                    cv.convolver_runtime_coeffs2cbuf(parts[k].ctypes.data_as(C.c_void_p), C.c_void_p(addr[rw[k]]))
                finally:
                    os._exit(0)
            assert os.waitpid(pid, 0)[1] == 0
        for j, e in enumerate(engines):
            st, raw = e.block(blk)
            assert st == 0
            outs[j].append(raw)
        assert engines[0].window_blocks == 4, k
    if lazy:
        rig.model_act(sw, ("coeff", fsw, key))
    for k in sorted(rw):
        rig.model_act(k, ("rewrite", key, rw[k], parts[k].astype(np.float64)))
    if not lazy:                             # the float32 rendering is what both engines hold
        rig.model[0].segs[0][1]["taps"] = h.astype(np.float64)
    want = rig.expect(blocks)
    for j, e in enumerate(engines):
        hold(xr.decode(np.concatenate(outs[j]), rig.outfmt, O), want, str(j))
        e.close()


# ------------------------------------------------------------------ f. integer outputs and status

@pytest.mark.parametrize("fmt", ["S16_LE", "S24_LE", "S32_LE"])
def test_integer_outputs_and_overflow_records(monkeypatch, fmt):
    N, I, O = 11, 8, 8
    sb = xr.FORMATS[fmt][1]
    full = float(1 << (8 * sb - 1))
    for seed in range(10):
        rig = Rig(N, I, O, seed=91 + 100 * seed, outfmt=fmt)
        blocks = blocks_for(rig, N + 2, seed=seed, amplitude=0.3)
        x = xr.decode(np.concatenate(blocks), rig.infmt, I)
        y = xr.output(x, rig.model, L, N, O, len(blocks))
        g = 0.6 / np.sqrt((y[:, [2, 5]] ** 2).mean())           # outputs 2 and 5 clip now and then
        for f in rig.model:
            if f.o in (2, 5):
                f.segs[0][1]["taps"] = f.segs[0][1]["taps"] * g
                rig.sets[(f.o, f.i)] = f.segs[0][1]["taps"]
        y = xr.output(x, rig.model, L, N, O, len(blocks))
        u = y * full + 0.5
        # the clip decisions must not hang on float32 rounding: no sample within 5e-6 of full scale
        if np.abs(np.abs(u) - full).min() > 5e-6 * full:
            break
    else:
        pytest.fail("no seed keeps every sample 5e-6 of full scale away from the clip level")
    want, ofs, st = xr.encode(y, fmt, L)
    # samples within 0.05 LSB of a rounding threshold (float32 carries ~1e-6 of the level) may land
    # either way; exact everywhere else.  For 24 and 32
    # bits float32 itself carries fewer bits than the sample: a bound relative to full scale there
    near = np.abs((u - np.round(u))) < 0.05
    assert st == [0] * len(blocks)
    assert ofs[2].n_overflows > 0 and ofs[0].n_overflows == 0
    for long in (True, False):
        e = rig.engine(monkeypatch, long)
        out = []
        for b in blocks:
            s, raw = e.block(b)
            assert s == 0 and e.window_blocks == (4 if long else 2)
            out.append(raw)
        got = np.rint(xr.decode(np.concatenate(out), fmt, O) * float(1 << (8 * sb - 1))).astype(np.int64)
        diff = np.abs(got - want)
        if sb == 2:
            assert diff[~near].max() == 0 and diff.max() <= 1, long
        else:
            assert diff.max() <= 2e-6 * full, (long, diff.max())
        for c in range(O):
            g = e.overflow(c)
            assert g.n_overflows == ofs[c].n_overflows, (long, c)
            assert abs(g.intlargest - ofs[c].intlargest) <= (1 if sb == 2 else 2e-6 * full), (long, c)
            if ofs[c].n_overflows:
                assert g.largest == pytest.approx(ofs[c].largest, rel=1e-5), (long, c)
            assert g.max == pytest.approx(ofs[c].max, rel=1e-5), (long, c)
        e.close()


def test_nan_input_sets_the_status_bit(monkeypatch):
    N, I, O = 8, 8, 8
    rig = Rig(N, I, O, seed=111, infmt="FLOAT_LE")
    blocks = blocks_for(rig, N + 2)
    blocks[N][100, 3] = np.nan
    for long in (True, False):
        e = rig.engine(monkeypatch, long)
        sts = []
        for b in blocks:
            sts.append(e.block(b)[0])
            assert e.window_blocks == (4 if long else 2)
        assert sts[:N] == [0] * N and all(s & bf.ST_NONFINITE for s in sts[N:]), (long, sts)
        e.close()


@pytest.mark.parametrize("env", [{"BFHIP_OVERLAP": "0", "BFHIP_DEFER": "0"}, {"BFHIP_OVERLAP": "0", "BFHIP_DEFER": "1"},
                                 {"BFHIP_OVERLAP": "1"}])
def test_safety_limit_status_at_the_first_block_over_it(monkeypatch, env):
    """set_safety_limit on FLOAT_LE outputs: BFHIP_ST_SAFETY comes back from the block call of the
    first output block in which the model exceeds the limit -- not earlier, not later -- in every
    schedule (block() launches what output_lag owes before it returns)"""
    N, I, O = 8, 8, 8
    rig = Rig(N, I, O, seed=181)
    K = N + 2
    blocks = blocks_for(rig, K, amplitude=0.02) + blocks_for(rig, 3, seed=8, amplitude=0.3)
    y = rig.expect(blocks)
    peak = np.abs(y).reshape(len(blocks), L, O).max(axis=(1, 2))
    below, above = peak[:K].max(), peak[K]
    assert above > 2.0 * below, (below, above)          # a clear margin on both sides of the limit
    limit = float(np.sqrt(below * above))
    for long in (True, False):
        e = rig.engine(monkeypatch, long, env)
        e.set_safety_limit(limit)
        sts = []
        for b in blocks[:K + 1]:
            sts.append(e.block(b)[0])
            assert e.window_blocks == (4 if long else 2)
        assert sts[:K] == [0] * K and sts[K] & bf.ST_SAFETY, (long, e.output_lag, sts)
        e.close()


def test_input_map_with_mute_and_sample_delay(monkeypatch):
    """two virtual inputs read physical channel 0: one delayed by 301 samples, the other muted
    halfway.  Nothing excludes input maps from the long plan; if the engine falls back that is
    recorded by the assertion on window_blocks and the outputs are checked either way"""
    N, I, O = 8, 8, 8
    v2p = [0, 0, 1, 2, 3, 4, 5, 6]
    n_phys = 7
    m = N + 2

    def setup(e):
        e.map_channels(0, v2p)
        e.set_interleaved_phys(0, "S24_4LE", n_phys)
        e.set_maxdelay(0, 1, 1000)
        e.set_delay(0, 1, 301)

    rig = Rig(N, I, O, seed=121)
    blocks = cases.raw_blocks(12, 2 * N + 2, L, n_phys, "S24_4LE")
    got, wins_seen = {}, {}
    for long in (True, False):
        e = rig.engine(monkeypatch, long, setup=setup)
        out = []
        wins = []
        for k, b in enumerate(blocks):
            if k == m:
                e.set_mute(0, 0, 1)
            s, raw = e.block(b)
            assert s == 0
            out.append(raw)
            wins.append(e.window_blocks)
        got[long] = xr.decode(np.concatenate(out), rig.outfmt, O)
        wins_seen[long] = wins
        e.close()
    x = xr.virtual_inputs(xr.decode(np.concatenate(blocks), "S24_4LE", n_phys), v2p, delay={1: 301},
                          mute_from={0: m}, L=L)
    want = xr.output(x, rig.model, L, N, O, len(blocks))
    assert set(wins_seen[False]) == {2}
    assert set(wins_seen[True]) == {4}, wins_seen[True]
    for long in (True, False):
        hold(got[long], want, str(long))


# ------------------------------------------------------------------ g. schedules

@pytest.mark.parametrize("env,mode", [({"BFHIP_OVERLAP": "0", "BFHIP_DEFER": "0"}, 0),
                                      ({"BFHIP_OVERLAP": "0", "BFHIP_DEFER": "1"}, 2),
                                      ({"BFHIP_OVERLAP": "1"}, 3)])
def test_schedules(monkeypatch, env, mode):
    N, I, O = 11, 8, 8
    rig = Rig(N, I, O, seed=131, n_extra=1)
    rng = np.random.default_rng(13)
    actions = {N + 1: [("coeff", 9, ("x", 0))], N + 3: [("rewrite", (2, 2), 10, _ir(int(rng.integers(1 << 30)), L, I))]}
    blocks = blocks_for(rig, N + 6)
    e = rig.engine(monkeypatch, True, env)
    assert e.block_mode == mode and e.output_lag == {0: 0, 2: 1, 3: 2}[mode]
    e.close()
    # block_dev on a long engine, the same control calls: block k's output pass is launched by call
    # k + output_lag (before that its buffer is untouched, even with the device idle) or by flush; the
    # bits must be block()'s (both() below builds its engines from the same sets: run this first)
    import torch
    e = rig.engine(monkeypatch, True, env)
    lag = e.output_lag
    fill = 0x5A
    outs = [torch.full((e.out_bytes,), fill, dtype=torch.uint8, device="cuda") for _ in blocks]
    srcs = [torch.from_numpy(np.ascontiguousarray(b).view(np.uint8).ravel().copy()).cuda() for b in blocks]
    torch.cuda.synchronize()
    for k in range(len(blocks)):
        for a in actions.get(k, ()):
            rig.act(e, a)
        e.block_dev(srcs[k], outs[k])
        assert e.window_blocks == 4, k
        torch.cuda.synchronize()
        # owed, not launched yet (a call that rebuilds the plan launches whatever was owed first)
        owed = range(k, k + 1) if (k in actions and lag) else range(max(0, k - lag + 1), k + 1)
        for j in owed:
            assert bool((outs[j] == fill).all()), (k, j, lag)
    e.flush()
    assert e.sync() == 0
    got_dev = np.concatenate([o.cpu().numpy() for o in outs])
    e.close()
    got_long, _, _ = both(monkeypatch, rig, blocks, actions, env)
    assert np.array_equal(got_dev, np.frombuffer(got_long.astype(np.float32).tobytes(), np.uint8))


# ------------------------------------------------------------------ h. real time

@pytest.mark.parametrize("flags", [0, bf.RT_COPY_ENGINE, bf.RT_OVERLAP])
def test_real_time_mode(monkeypatch, flags):
    """graph replay (BlockState read by the long MAC and io_long_kernel), with a set_coeff and a
    rewrite between periods; bit for bit what block() gives, and the model"""
    N, I, O = 8, 8, 8
    cv = _cv()
    rig = Rig(N, I, O, seed=141, n_extra=1)
    rng = np.random.default_rng(14)
    actions = {N + 2: [("coeff", 12, ("x", 0))],
               N + 5: [("rewrite", (4, 1), 7, _ir(int(rng.integers(1 << 30)), L, I))],
               2 * N + 1: [("rewrite", (4, 1), 2, _ir(int(rng.integers(1 << 30)), L, I))]}
    # set (2, 6) lives in shared memory; a forked process rewrites its partition 6 (the last long one)
    wkey, wblk, wt = (2, 6), 6, N + 7
    wpart = _ir(int(rng.integers(1 << 30)), L, I).astype(np.float32)
    h = rig.sets[wkey].astype(np.float32)
    shm = mmap.mmap(-1, N * 2 * L * 4)
    base = np.frombuffer(shm, np.float32)
    addr = [base[b * 2 * L:].ctypes.data for b in range(N)]

    def hook(e):
        for b in range(N):
            t = np.ascontiguousarray(h[b * L:(b + 1) * L])
            assert cv.convolver_coeffs2cbuf(t.ctypes.data_as(C.c_void_p), L, 1.0, C.c_void_p(addr[b])) == addr[b]
        e.cid[wkey] = e.add_coeff_processed_blocks(addr, watch=True)

    blocks = blocks_for(rig, 2 * N + 6)
    res = {}
    for rt in (flags, None):
        e = rig.engine(monkeypatch, True, sets_hook=hook)
        assert e.window_blocks == 4
        if rt is not None:
            e.rt_begin(rt)
        outs = []
        pending = 0
        for k, b in enumerate(blocks):
            for a in actions.get(k, ()):
                rig.act(e, a)
            if k == wt:
                pid = os.fork()
                if pid == 0:
                    try:
                        cv.convolver_runtime_coeffs2cbuf(wpart.ctypes.data_as(C.c_void_p), C.c_void_p(addr[wblk]))
                    finally:
                        os._exit(0)
                assert os.waitpid(pid, 0)[1] == 0
            if rt is None:
                outs.append(e.block(b))
            elif rt & bf.RT_OVERLAP:
                e.rt_submit(b)
                pending += 1
                if pending == 2:
                    outs.append(e.rt_wait())
                    pending -= 1
            else:
                outs.append(e.rt_block(b))
            assert e.window_blocks == 4, k
        while pending:
            outs.append(e.rt_wait())
            pending -= 1
        if rt is not None:
            stats = e.rt_stats()
            if rt & bf.RT_OVERLAP:           # no replay in this mode (bfhip.h): every period launched directly
                assert stats["graph"] == 0 and stats["direct"] == len(blocks), stats
            else:
                assert stats["graph"] > 0, stats
            e.rt_end()
        assert [s for s, _ in outs] == [0] * len(blocks)
        res[rt] = np.concatenate([r for _, r in outs])
        e.close()
    assert np.array_equal(res[flags], res[None])
    actions.setdefault(wt, []).append(("rewrite", wkey, wblk, wpart.astype(np.float64)))
    want = rig.expect(blocks, actions)
    hold(xr.decode(res[flags], rig.outfmt, O), want)


# ------------------------------------------------------------------ i. counter wrap

@pytest.mark.parametrize("overlap", ["0", "1"])
def test_counter_wrap(monkeypatch, overlap):
    """BFHIP_TEST_WRAP_PERIODS=2 on the long plan, R = N and R = N + 1 (ping-pong), column delays"""
    N, I, O = 8, 5, 8
    rig = Rig(N, I, O, seed=151, delays={0: 2, 1: N - 1, 2: 0, 3: 5, 4: 1})
    env = {"BFHIP_TEST_WRAP_PERIODS": "2", "BFHIP_OVERLAP": overlap, "BFHIP_DEFER": "0"}
    e = rig.engine(monkeypatch, True, env)
    R = e.ring_depth
    assert R == (N if overlap == "0" else N + 1) and e.window_blocks == 4
    period = N if R == N else N * R
    n_wraps = 3
    n_blocks = (n_wraps * 2 * period + 2 * R + 3)
    blocks = blocks_for(rig, n_blocks)
    seen, out = [], []
    for b in blocks:
        s, raw = e.block(b)
        assert s == 0
        out.append(raw)
        seen.append(e.blockcounter)
    wrapped = sum(1 for a, b in zip(seen, seen[1:]) if b < a)
    assert wrapped >= n_wraps, seen
    assert e.window_blocks == 4
    e.close()
    want = rig.expect(blocks)
    hold(xr.decode(np.concatenate(out), rig.outfmt, O), want)


def test_counter_wrap_inside_replay(monkeypatch):
    N, I, O = 8, 8, 8
    rig = Rig(N, I, O, seed=161, delays={3: 2, 6: N - 2})
    e = rig.engine(monkeypatch, True, {"BFHIP_TEST_WRAP_PERIODS": "1"})
    R = e.ring_depth
    assert R in (N, N + 1)
    period = N if R == N else N * R
    blocks = blocks_for(rig, 3 * period + 2 * R + 5)          # three wraps
    e.rt_begin(0)
    out, seen = [], []
    for b in blocks:
        s, raw = e.rt_block(b)
        assert s == 0
        out.append(raw)
    assert e.rt_stats()["graph"] > 0 and e.window_blocks == 4
    e.rt_end()
    # the host's counter after the replayed periods: wrap by `period` at period + 2R (advance())
    c, wraps = 0, 0
    for _ in blocks:
        c += 1
        if c >= period + 2 * R:
            c -= period
            wraps += 1
    assert wraps >= 3 and e.blockcounter == c, (wraps, c, e.blockcounter)
    e.close()
    hold(xr.decode(np.concatenate(out), rig.outfmt, O), rig.expect(blocks))


# ------------------------------------------------------------------ j. long chunks

@pytest.mark.parametrize("chunks", ["2", "4"])
def test_long_chunks(monkeypatch, chunks):
    rig = Rig(11, 8, 8, seed=171)
    both(monkeypatch, rig, blocks_for(rig, 14), env={"BFHIP_LONG_CHUNKS": chunks})


# ------------------------------------------------------------------ k. the default gate, real data

def test_default_gate_with_a_gigabyte_of_distinct_sets(monkeypatch):
    """BFHIP_LONG_WINDOW unset, 16 x 16 at N = 64 from distinct device sets (1 GiB of spectra): the
    long plan, a column delay and a set_coeff partway, every output against float64 torch.fft"""
    import torch
    monkeypatch.delenv("BFHIP_LONG_WINDOW", raising=False)
    for k in ("BFHIP_OVERLAP", "BFHIP_DEFER", "BFHIP_LONG_CHUNKS"):
        monkeypatch.delenv(k, raising=False)
    I = O = 16
    N = 64
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5)
    decay = torch.exp(-torch.arange(L * N, device=dev, dtype=torch.float64) / (L * N / 6.0))
    e = bf.Engine(L, N, 4, I, O)
    e.set_interleaved(0, "S24_4LE")
    e.set_interleaved(1, "FLOAT_LE")
    e.reserve_coeffs(float(I * O + 1) * N * 2 * L * 4)
    taps = {}
    d_col = {5: 3}
    for key in [(o, i) for o in range(O) for i in range(I)] + ["alt"]:
        h = torch.randn(L * N, device=dev, dtype=torch.float64, generator=g) * decay
        h = (h / (h.abs().sum() * I)).to(torch.float32)
        taps[key] = h
        c = e.add_coeff_dev(h, L * N)
        taps[key, "c"] = c
    for o in range(O):
        for i in range(I):
            e.add_filter(in_ch=[i], out_ch=[o], coeff=taps[(o, i), "c"], delayblocks=d_col.get(i, 0))
    torch.cuda.synchronize()
    e.finalize()
    assert e.window_blocks == 4
    n_blocks, sw, fsw = 2 * N + 2, N + 5, 7 * I + 9
    blocks = cases.raw_blocks(3, n_blocks, L, I, "S24_4LE")
    out = []
    for k, b in enumerate(blocks):
        if k == sw:
            e.set_coeff(fsw, taps["alt", "c"])
        s, raw = e.block(b)
        assert s == 0
        assert e.window_blocks == 4, k
        out.append(raw)
    e.close()
    got = torch.from_numpy(xr.decode(np.concatenate(out), "FLOAT_LE", O)).to(dev)
    x = torch.from_numpy(xr.decode(np.concatenate(blocks), "S24_4LE", I)).to(dev)
    n = n_blocks * L
    nfft = 1 << (n + L * N).bit_length()
    X = [torch.fft.rfft(x[:, i], nfft) for i in range(I)]
    for o in range(O):
        acc = torch.zeros(nfft // 2 + 1, dtype=torch.complex128, device=dev)
        acc_alt = dH = None
        for i in range(I):
            d = d_col.get(i, 0)
            h = taps[(o, i)].to(torch.float64)[:(N - d) * L]
            Xd = torch.fft.rfft(torch.cat([torch.zeros(d * L, dtype=torch.float64, device=dev), x[:n - d * L, i]]), nfft) if d else X[i]
            acc += Xd * torch.fft.rfft(h, nfft)
            if o * I + i == fsw:
                dH = Xd * (torch.fft.rfft(taps["alt"].to(torch.float64)[:(N - d) * L], nfft) - torch.fft.rfft(h, nfft))
        y = torch.fft.irfft(acc, nfft)[:n]
        if dH is not None:
            acc_alt = acc + dH
        if acc_alt is not None:
            y2 = torch.fft.irfft(acc_alt, nfft)[:n]
            y = torch.cat([y[:sw * L], y2[sw * L:]])
        for k in range(n_blocks):
            s = slice(k * L, (k + 1) * L)
            err = float(torch.sqrt(((got[s, o] - y[s]) ** 2).sum() / (y[s] ** 2).sum()))
            assert err <= TOL_BLOCK, (o, k, err)
