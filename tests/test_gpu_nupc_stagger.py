"""GPU: staggered switches of the non-uniform convolver (include/bfhip_nupc.h,
BFHIP_NUPC_SWITCH_STAGGERED): every segment switches at its own next launch, so a switch is heard in
the period it is committed in.  Reference: the float64 model of tests/nupc_stagger_ref.py (checked on
its own in tests/test_nupc_stagger_model.py) -- per-segment full-history convolutions blended at the
per-segment switch frames -- at float32 1e-5 / float64 1e-12 relative RMS over the whole run and
per 64-frame block.  Every impulse response is flat noise over the whole schedule and the sets of a
filter differ in every segment, so a segment switched at the wrong frame shows."""
import ctypes as C

import numpy as np
import pytest

import cases
import nupc_stagger_ref as sr
from nupc_stagger_ref import SMALL, ZERO

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
EINVAL, ESTATE = -1, -5


class Rig:
    """a 2x2 crossbar (sr.Crossbar's data) on the device, in staggered mode unless told otherwise"""

    def __init__(self, hip, rs, n_sets, seed, sched=SMALL, n_frames=0, mode=1, gains=False):
        self.hip, self.rs, self.dt = hip, rs, (np.float32 if rs == 4 else np.float64)
        self.sched = sched
        self.cb = cb = sr.Crossbar(sched, n_sets, seed, n_frames, self.dt)
        self.nu = nu = hip.Nupc(sched[0], sched[1], rs, 2, 2)
        assert nu.taps == cb.taps
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, FF[rs])
        for f in range(4):
            nu.add_filter(f % 2, f // 2, cb.h[f][0], in_scale=cb.in_scale[f], out_scale=cb.out_scale[f])
            for j in range(1, n_sets):
                assert nu.add_coeff(f, cb.h[f][j]) == j
        if gains:
            nu.reserve_filter_gain()
        if mode is not None:
            assert nu.switch_mode() == hip.SWITCH_ALIGNED          # the default
            nu.set_switch_mode(mode)
            assert nu.switch_mode() == mode
        nu.finalize()
        self.L0 = nu.L0
        self.asg = [(0, 1.0)] * 4          # the model's assignment: (index into cb.h[f], gain)
        self.req, self.F = {}, self.L0
        self.commits, self.busy, self.want_busy = [], [], []

    def request(self, sets=None, gains=None, F=None, model_sets=None):
        """queue a group; model_sets: the model's index where it differs from the device's set"""
        if F is not None:
            self.F = F
            self.nu.set_crossfade(F)
        assert not self.nu.switch_busy()
        for f, c in (sets or {}).items():
            self.nu.set_coeff(f, c)
            self.req.setdefault(f, {})["set"] = (model_sets or {}).get(f, c)
        for f, g in (gains or {}).items():
            self.nu.set_filter_gain(f, g)
            self.req.setdefault(f, {})["gain"] = g

    def run(self, actions=None, after=None, blocks=None):
        """block by block; actions[b](rig) runs before block call b, after(rig, b) behind it.  Checks
        the reported switch frames of every commit and records the busy flag after every call."""
        nu, L0, n_seg = self.nu, self.L0, len(self.sched[0])
        got = []
        if not self.commits:
            assert nu.switch_frame() == -1 and [nu.switch_frame_segment(k) for k in range(n_seg)] == [-1] * n_seg
        for b in range(blocks or len(self.cb.x) // L0):
            if actions and b in actions:
                actions[b](self)
            st, raw = nu.block(self.cb.x[b * L0:(b + 1) * L0])
            assert st == 0
            got.append(raw)
            new = [(r.get("set", a[0]), r.get("gain", a[1])) for a, r in
                   zip(self.asg, (self.req.get(f, {}) for f in range(4)))]
            self.req = {}
            if new != self.asg:
                self.commits.append((b * L0, self.F, new))
                self.asg = new
                assert nu.switch_frame() == b * L0
                assert [nu.switch_frame_segment(k) for k in range(n_seg)] == sr.switch_frames(self.sched, b * L0)
            self.busy.append(nu.switch_busy())
            if self.commits:
                t_req, F, _ = self.commits[-1]
                self.want_busy.append(sr.busy_after(self.sched, (b + 1) * L0, sr.switch_frames(self.sched, t_req), F))
            else:
                self.want_busy.append(False)
            if after:
                after(self, b)
        return np.concatenate(got)

    def want(self):
        return self.cb.model(self.commits)


def _frames(raw, dt):
    return np.frombuffer(raw.tobytes(), dt).reshape(-1, 2).astype(np.float64)


def _check(got, want, rs, L0=64):
    err = cases.rel_rms(got, want)
    print("rel rms over the run: %.3g" % err)
    assert err <= TOL[rs]
    for b in range(0, len(want), L0):
        if np.abs(want[b:b + L0]).max() > 0:
            assert cases.rel_rms(got[b:b + L0], want[b:b + L0]) <= TOL[rs], b // L0


def _all(c):
    return {f: c for f in range(4)}


# ---- 1. hard switches

@pytest.mark.parametrize("rs", [4, 8])
def test_hard_switch_in_the_very_next_period(hip, rs):
    """F = 0; requests at blocks 5, 37, 83 (off the 512-frame grid) and 120 (on it)"""
    rig = Rig(hip, rs, 2, 11 + rs, n_frames=64 * 160)
    plan = ((5, 1), (37, 0), (83, 1), (120, 0))
    segs = {}

    def after(r, b):
        if b == 5:
            segs[5] = [r.nu.switch_frame_segment(k) for k in range(4)]

    got = _frames(rig.run({b: (lambda r, c=c: r.request(_all(c), F=0)) for b, c in plan}, after), rig.dt)
    assert [c[0] for c in rig.commits] == [b * 64 for b, _ in plan]
    assert segs[5] == [320, 384, 640, 896]
    assert not any(rig.busy)
    _check(got, rig.want(), rs)
    # heard at once: the first period after each request already differs from the output without
    # that switch (the model's margin is >= 0.29, tests/test_nupc_stagger_model.py)
    for i, (t, _, _) in enumerate(rig.commits):
        y_old = rig.cb.model(rig.commits[:i])
        assert cases.rel_rms(got[t:t + 64], y_old[t:t + 64]) > 0.1, t // 64


# ---- 2. cross-fades

@pytest.mark.parametrize("sched", [SMALL, ZERO], ids=["small", "zero"])
@pytest.mark.parametrize("F", [2, 64, 5 * 64 + 3, 700])
def test_crossfade_per_segment(hip, F, sched):
    """F = 700 is longer than the longest block: several blocks of a segment run under both
    assignments.  The second request comes off the grid of the long segments."""
    rig = Rig(hip, 4, 2, 23, sched=sched, n_frames=64 * 100)
    acts = {7: lambda r: r.request(_all(1), F=F), 61: lambda r: r.request(_all(0))}
    got = _frames(rig.run(acts), rig.dt)
    assert [c[:2] for c in rig.commits] == [(7 * 64, F), (61 * 64, F)]
    assert rig.busy == rig.want_busy
    assert any(rig.busy)
    _check(got, rig.want(), 4)


def test_crossfade_float64(hip):
    rig = Rig(hip, 8, 2, 29, n_frames=64 * 60)
    got = _frames(rig.run({9: lambda r: r.request({0: 1, 3: 1}, F=5 * 64 + 3)}), rig.dt)
    assert rig.busy == rig.want_busy
    _check(got, rig.want(), 8)


# ---- 3. back-to-back switches

@pytest.mark.parametrize("sched", [SMALL, ZERO], ids=["small", "zero"])
def test_switch_as_soon_as_busy_clears(hip, sched):
    """F = 64, a new switch whenever the previous one has left busy, for the whole run: background
    blocks of one switch are still pending when the next is committed"""
    rig = Rig(hip, 4, 3, 33, sched=sched, n_frames=64 * 100)
    rig.nu.set_crossfade(64)
    rig.F = 64

    def after(r, b):
        if b >= 3 and not r.nu.switch_busy():
            r.request(_all((len(r.commits) + 1) % 3))

    got = _frames(rig.run(after=after), rig.dt)
    # a switch is busy until its longest segment's next launch at the latest: Lmax / L0 periods,
    # and the request is committed by the call after that
    assert len(rig.commits) >= (100 - 4) // (sched[0][-1] // 64 + 1)
    assert rig.busy == rig.want_busy
    _check(got, rig.want(), 4)


def test_second_hard_switch_replaces_the_first_in_long_segments(hip):
    """two F = 0 switches in consecutive periods: the 256 and 512 segments have not launched in
    between, keep their switch frame and run the later assignment from it"""
    rig = Rig(hip, 8, 3, 37, n_frames=64 * 60)
    seg = []

    def after(r, b):
        if b in (5, 6):
            seg.append([r.nu.switch_frame_segment(k) for k in range(4)])

    acts = {5: lambda r: r.request(_all(1), F=0), 6: lambda r: r.request(_all(2), F=0)}
    got = _frames(rig.run(acts, after), rig.dt)
    assert seg == [[320, 384, 640, 896], [384, 512, 640, 896]]
    assert not any(rig.busy)
    _check(got, rig.want(), 8)


# ---- 4. gain-only switches

def test_gain_only_staggered_switch(hip):
    """one set per filter, reserve_filter_gain; a polarity flip, a silenced filter, and back"""
    rig = Rig(hip, 4, 1, 43, n_frames=64 * 100, gains=True)
    acts = {5: lambda r: r.request(gains={0: -1.0, 1: 0.0}, F=64),
            40: lambda r: r.request(gains={1: 0.5, 2: 2.0}, F=0),
            63: lambda r: r.request(gains={0: 1.0, 3: -0.25}, F=200)}
    got = _frames(rig.run(acts), rig.dt)
    assert [c[2] for c in rig.commits] == [[(0, -1.0), (0, 0.0), (0, 1.0), (0, 1.0)],
                                           [(0, -1.0), (0, 0.5), (0, 2.0), (0, 1.0)],
                                           [(0, 1.0), (0, 0.5), (0, 2.0), (0, -0.25)]]
    assert rig.nu.get_filter_gain(3) == -0.25
    assert rig.busy == rig.want_busy
    _check(got, rig.want(), 4)


# ---- 5. state rules

def test_state_rules(hip):
    L = hip.lib()
    rig = Rig(hip, 8, 2, 53, n_frames=64 * 90)
    nu, h = rig.nu, rig.nu.h
    fresh = (np.random.default_rng(7).standard_normal(nu.taps) / np.sqrt(nu.taps)).astype(np.float64)
    p = fresh.ctypes.data_as(C.c_void_p)
    seen = {}
    assert L.bfhip_nupc_set_switch_mode(h, 2) == EINVAL
    assert L.bfhip_nupc_set_switch_mode(h, -1) == EINVAL
    assert L.bfhip_nupc_switch_frame_segment(h, 4) < -1 and L.bfhip_nupc_switch_frame_segment(h, -1) < -1

    def req(r):
        r.request(_all(1), F=700)
        seen["queued"] = L.bfhip_nupc_set_switch_mode(h, hip.SWITCH_ALIGNED)

    def after(r, b):
        if b == 6:
            assert nu.switch_busy()
            seen["busy"] = L.bfhip_nupc_set_switch_mode(h, hip.SWITCH_ALIGNED)
            seen["old set, busy"] = L.bfhip_nupc_update_coeff(h, 1, 0, p, nu.taps)
            seen["new set, busy"] = L.bfhip_nupc_update_coeff(h, 1, 1, p, nu.taps)
            assert nu.switch_mode() == hip.SWITCH_STAGGERED
        if b == 40:
            assert not nu.switch_busy()
            nu.update_coeff(1, 0, fresh)                 # the old set is idle now
            r.cb.h[1].append(fresh)                      # the model's set 2 of filter 1
            nu.set_switch_mode(hip.SWITCH_STAGGERED)     # allowed again (and no change)

    acts = {6: req, 60: lambda r: r.request({1: 0}, F=0, model_sets={1: 2})}
    got = _frames(rig.run(acts, after), rig.dt)
    assert seen == {"queued": ESTATE, "busy": ESTATE, "old set, busy": ESTATE, "new set, busy": ESTATE}
    assert [c[2] for c in rig.commits] == [[(1, 1.0)] * 4, [(1, 1.0), (2, 1.0), (1, 1.0), (1, 1.0)]]
    assert rig.busy == rig.want_busy
    _check(got, rig.want(), 8)


# ---- 6. nothing else moves

def test_mode_alone_changes_no_byte(hip):
    """no switch ever requested: a staggered-mode convolver emits the bytes of a default one"""
    a = Rig(hip, 4, 2, 61, n_frames=64 * 40)
    b = Rig(hip, 4, 2, 61, n_frames=64 * 40, mode=None)
    assert np.array_equal(a.run(), b.run())


def test_explicit_aligned_is_the_default(hip):
    """through a cross-faded switch, bytes and switch frames"""
    outs, frames = [], []
    for mode in (0, None):
        rig = Rig(hip, 4, 2, 67, n_frames=64 * 70, mode=mode)
        nu, out = rig.nu, []
        for b in range(70):
            if b == 9:
                nu.set_crossfade(100)
                for f in range(4):
                    nu.set_coeff(f, 1)
            st, raw = nu.block(rig.cb.x[b * 64:(b + 1) * 64])
            assert st == 0
            out.append(raw)
        outs.append(np.concatenate(out))
        frames.append([nu.switch_frame()] + [nu.switch_frame_segment(k) for k in range(4)])
    assert np.array_equal(outs[0], outs[1])
    assert frames[0] == frames[1] and len(set(frames[0])) == 1 and frames[0][0] >= 9 * 64


def test_block_and_block_dev_same_bits(hip):
    import torch
    runs = []
    for dev in (False, True):
        rig = Rig(hip, 4, 2, 71, n_frames=64 * 70)
        nu = rig.nu
        out = []
        if dev:
            din = torch.empty(64 * 2 * 4, dtype=torch.uint8, device="cuda")
            dout = torch.empty(64 * 2 * 4, dtype=torch.uint8, device="cuda")
        for b in range(70):
            if b == 9:
                nu.set_crossfade(100)
                for f in range(4):
                    nu.set_coeff(f, 1)
            xb = rig.cb.x[b * 64:(b + 1) * 64]
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
        assert nu.switch_frame() == 9 * 64
        runs.append(np.concatenate(out))
    assert np.array_equal(runs[0], runs[1])
