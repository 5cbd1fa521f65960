"""CPU, float64, numpy only: the model of the staggered switches (tests/nupc_stagger_ref.py) that
the GPU tests compare against is itself checked -- the segments' slices add up to the full
convolution, the switch-frame formula is what a walk of the launch grid gives, the model with all
switch frames forced equal is the aligned cross-fade of tests/nupc_ref.py, and every hard switch the
GPU tests request is audible in the model's very first period."""
import numpy as np
import pytest

import cases
import nupc_ref
import nupc_stagger_ref as sr
from nupc_stagger_ref import SMALL, ZERO

DOUBLING = ([64, 128, 256, 512, 1024], [2, 2, 2, 2, 3])
LATE = ([64, 256], [5, 2])                      # a segment that starts later than it has to
A0 = [(0, 1.0)] * 4
A1 = [(1, 1.0)] * 4


@pytest.mark.parametrize("sched", [SMALL, ZERO, LATE])
def test_segment_slices_sum_to_the_full_convolution(sched):
    cb = sr.Crossbar(sched, 1, 3, 64 * 40)
    full = np.zeros((len(cb.x), 2))
    for f in range(4):
        full[:, f // 2] += sr.conv(cb.x[:, f % 2], cb.h[f][0], len(cb.x)) * cb.in_scale[f] * cb.out_scale[f]
    assert cases.rel_rms(cb.yseg(A0).sum(axis=0), full) <= 1e-13
    # and a gain scales its filter alone
    g = [(0, 1.0), (0, -2.0), (0, 0.0), (0, 1.0)]
    want = np.zeros_like(full)
    for f in range(4):
        want[:, f // 2] += sr.conv(cb.x[:, f % 2], cb.h[f][0], len(cb.x)) * cb.in_scale[f] * cb.out_scale[f] * g[f][1]
    assert cases.rel_rms(cb.yseg(g).sum(axis=0), want) <= 1e-13


@pytest.mark.parametrize("sched", [SMALL, ZERO, DOUBLING, LATE])
def test_switch_frames_are_the_launch_grid(sched):
    L0 = sched[0][0]
    for b in range(0, 70):
        t_req = b * L0
        t = sr.switch_frames(sched, t_req)
        assert t == sr.switch_frames_walk(sched, t_req), b
        assert t[0] == t_req and min(t) >= t_req
    assert sr.switch_frames(SMALL, 5 * 64) == [320, 384, 640, 896]


@pytest.mark.parametrize("F", [0, 2, 64, 323, 700])
def test_equal_switch_frames_reduce_to_the_aligned_crossfade(F):
    cb = sr.Crossbar(SMALL, 2, 5, 64 * 60)
    ys = [cb.yseg(A0), cb.yseg(A1)]
    for t in (0, 7 * 64, 896, 1001):
        got = sr.staggered(ys, [(0, F, 1)], SMALL, frames=lambda t_req, t=t: [t] * 4)
        want = nupc_ref.crossfade(ys[0].sum(axis=0), ys[1].sum(axis=0), t, F)
        assert cases.rel_rms(got, want) <= 1e-13
    # two switches in a row, the second back onto the first assignment
    got = sr.staggered(ys, [(0, F, 1), (0, 64, 0)], SMALL, frames=lambda t_req: [640] * 4)
    want = nupc_ref.crossfade(nupc_ref.crossfade(ys[0].sum(axis=0), ys[1].sum(axis=0), 640, F), ys[0].sum(axis=0), 640, 64)
    assert cases.rel_rms(got, want) <= 1e-13


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_hard_switches_are_heard_in_the_first_period(dt):
    """the requests of tests/test_gpu_nupc_stagger.py with F = 0, same seeds: the model's
    [t_req, t_req + L0) against the output without the switch"""
    rs = 4 if dt == np.float32 else 8
    cb = sr.Crossbar(SMALL, 2, 11 + rs, 64 * 160, dt)
    commits, prev = [], A0
    for b, c in ((5, 1), (37, 0), (83, 1), (120, 0)):
        new = [(c, 1.0)] * 4
        t = b * 64
        y_old = cb.model(commits)
        commits.append((t, 0, new))
        y = cb.model(commits)
        assert cases.rel_rms(y[t:t + 64], y_old[t:t + 64]) > 0.1, b
        assert np.array_equal(y[:t], y_old[:t])
        prev = new
    # the back-to-back pair: sets 1 at block 5 and 2 at block 6
    cb = sr.Crossbar(SMALL, 3, 37, 64 * 60)
    one = [(5 * 64, 0, [(1, 1.0)] * 4)]
    two = one + [(6 * 64, 0, [(2, 1.0)] * 4)]
    assert cases.rel_rms(cb.model(one)[320:384], cb.model([])[320:384]) > 0.1
    assert cases.rel_rms(cb.model(two)[384:448], cb.model(one)[384:448]) > 0.1
    # the second replaces the first in the segments whose next launch is the same: set 1 is never
    # heard from them
    t1, t2 = sr.switch_frames(SMALL, 320), sr.switch_frames(SMALL, 384)
    assert [a == b for a, b in zip(t1, t2)] == [False, False, True, True]
    y2 = cb.yseg([(2, 1.0)] * 4)
    y0 = cb.yseg(A0)
    tail = np.where(np.arange(len(cb.x))[:, None] >= 896, y2[3], y0[3])
    skipped = sr.staggered([cb.yseg(A0), cb.yseg([(1, 1.0)] * 4), y2], [(320, 0, 1), (384, 0, 2)], SMALL)
    rest = sr.staggered([y0[:3], cb.yseg([(1, 1.0)] * 4)[:3], y2[:3]], [(320, 0, 1), (384, 0, 2)],
                        (SMALL[0][:3], SMALL[1][:3]))
    assert cases.rel_rms(skipped, rest + tail) <= 1e-13


def test_busy_rule():
    # F = 0: never busy, whatever the request block
    for b in range(40):
        t = sr.switch_frames(SMALL, b * 64)
        assert not any(sr.busy_after(SMALL, e, t, 0) for e in range((b + 1) * 64, (b + 40) * 64, 64))
    # SMALL, request at block 5, F = 64: the 512 segment's dual block is launched by the call that
    # completes frame 512; busy through the call before it
    t = sr.switch_frames(SMALL, 320)
    seq = [sr.busy_after(SMALL, e, t, 64) for e in range(384, 704, 64)]
    assert seq == [True, True, False, False, False]
