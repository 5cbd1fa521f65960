"""GPU: per-filter gains as part of a switch, the ramped output gain and the peak reset of the
non-uniform convolver (include/bfhip_nupc.h).  Reference: the float64 model of tests/nupc_ref.py:
the full-history convolution under each assignment (filter -> (set, gain), the gain multiplied
into out_scale), blended by the header's definition at the switch frame the library reports,
times the per-frame output gain g[t] of the header's ramp definition, encoded period by period.
Float outputs: relative RMS 1e-5 (float32) / 1e-12 (float64) over the run and per 64-frame block,
all-zero blocks compared for equality.  Integer outputs: within one count of the model's unrounded
value.  The 2x2 rig of tests/test_gpu_nupc_switch.py at its smallest schedule: segment offsets 0 /
128 / 384 / 896, so every segment sees a change at a different position of its own block."""
import numpy as np
import pytest

import bforacle as bo
import cases
import nupc_ref as nr
from nupc_chain_ref import GainRamp

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])     # offsets 0, 128, 384, 896
MAX_OFF = 896
EINVAL, ESTATE = -1, -5
L0 = 64


class Rig:
    """a 2x2 crossbar (filter f = 2 * out + in) with n_sets flat-noise impulse responses per filter;
    an assignment is a list of (set, gain) per filter"""

    def __init__(self, hip, rs, seed, n_blocks, n_sets=1, reserve=True, outfmt=None, init_gain=None, dither=(),
                 subdelay=None, out_gain=None, amp=0.1):
        self.hip, self.rs, self.dt = hip, rs, (np.float32 if rs == 4 else np.float64)
        self.nu = nu = hip.Nupc(SMALL[0], SMALL[1], rs, 2, 2)
        self.outfmt = outfmt or FF[rs]
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, self.outfmt)
        self.fmts = bo.interleaved_formats(self.outfmt, 2)
        self.dither = tuple(dither)
        if dither:
            nu.enable_dither(list(dither), 300)
        self.half = subdelay
        if subdelay:
            nu.enable_subdelay(subdelay)
            for c, v in enumerate((37, -62)):
                nu.set_subdelay(hip.OUT, c, v)
        rng = np.random.default_rng(seed)
        self.h = [[(rng.standard_normal(nu.taps) / np.sqrt(nu.taps)).astype(self.dt) for _ in range(n_sets)]
                  for _ in range(4)]
        self.in_scale = [0.5 if f % 2 else 1.0 for f in range(4)]
        self.out_scale = [-1.0 if f // 2 else 1.0 for f in range(4)]
        for f in range(4):
            nu.add_filter(f % 2, f // 2, self.h[f][0], in_scale=self.in_scale[f], out_scale=self.out_scale[f])
            for j in range(1, n_sets):
                assert nu.add_coeff(f, self.h[f][j]) == j
        self.asg0 = [(0, 1.0)] * 4
        if init_gain:
            for f, g in init_gain.items():
                nu.set_filter_gain(f, g)
                self.asg0[f] = (0, g)
        if reserve:
            nu.reserve_filter_gain()
        self.g0 = [1.0, 1.0]
        for c, g in (out_gain or {}).items():
            nu.set_output_gain(c, g)
            self.g0[c] = g
        nu.finalize()
        self.n = n_blocks * L0
        self.x = (rng.standard_normal((self.n, 2)) * amp).astype(self.dt)
        self._c = {}

    # ---- model
    def y(self, asg):
        """full-history float64 output under an assignment: nupc_ref.convolve with out_scale * gain"""
        out = np.zeros((self.n, 2))
        for f, (s, g) in enumerate(asg):
            if (f, s) not in self._c:
                self._c[(f, s)] = nr.conv(self.x[:, f % 2], self.h[f][s], self.n)
            out[:, f // 2] += self._c[(f, s)] * (self.in_scale[f] * (self.out_scale[f] * g))
        return out

    def blended(self):
        out = self.y(self.asg0)
        for _, t, F, asg in self.switches:
            out = nr.crossfade(out, self.y(asg), t, F)
        return out

    def want_raw(self, overflow=None, first_block=0):
        """the expected raw stream and overflow structs (from first_block on)"""
        y = self.blended() * self.g
        if self.half:
            y = y / np.array([f.scale for f in self.fmts])
            y = np.stack([self._fir(y[:, c], (37, -62)[c]) for c in range(2)], axis=1)
            y = y * np.array([f.scale for f in self.fmts])
        assert not (first_block and self.dither)
        raw, of, _ = nr.encode(y[first_block * L0:], self.fmts, L0, dither=self.dither, rate=300, overflow=overflow)
        return raw, of

    def _fir(self, x, v):
        half = self.half
        taps = np.zeros(2 * half + 1, self.dt)
        assert self.hip.lib().bfhip_selftest_subdelay_filter(half, v, self.rs, taps.ctypes.data) == 2 * half + 1
        return np.convolve(np.concatenate([np.zeros(2 * half), x]), taps.astype(np.float64), mode="valid")

    # ---- run
    def run(self, actions=None, after=None, dev=False):
        """block by block; actions[b](rig) runs before block call b.  Tracks the committed switches
        [(block, t_sw, F, assignment)] and the per-frame output gain self.g"""
        nu = self.nu
        self.asg, self.req, self.F, self.switches = list(self.asg0), {}, L0, []
        self.gr = GainRamp(self.n, L0, self.g0)
        self.g = self.gr.g
        got, t_last = [], nu.switch_frame()
        if dev:
            import torch
            din = torch.empty(nu.in_bytes, dtype=torch.uint8, device="cuda")
            dout = torch.empty(nu.out_bytes, dtype=torch.uint8, device="cuda")
        for b in range(self.n // L0):
            if actions and b in actions:
                actions[b](self)
            self._commit_gain(b)
            xb = self.x[b * L0:(b + 1) * L0]
            if dev:
                din.copy_(torch.from_numpy(xb.view(np.uint8).ravel().copy()))
                torch.cuda.synchronize()
                nu.block_dev(din, dout)
                assert nu.sync() == 0
                raw = dout.cpu().numpy().copy()
            else:
                st, raw = nu.block(xb)
                assert st == 0
            got.append(raw)
            t = nu.switch_frame()
            if t != t_last:
                new = list(self.asg)
                for f, (s, g) in self.req.items():
                    new[f] = (new[f][0] if s is None else s, new[f][1] if g is None else g)
                self.switches.append((b, t, self.F, new))
                self.asg, t_last = new, t
            self.req = {}
            if after:
                after(self, b)
        return np.concatenate(got)

    def request(self, sets=None, gains=None, F=None):
        if F is not None:
            self.F = F
            self.nu.set_crossfade(F)
        assert not self.nu.switch_busy()
        for f, c in (sets or {}).items():
            self.nu.set_coeff(f, c)
            self.req[f] = (c, self.req.get(f, (None, None))[1])
        for f, g in (gains or {}).items():
            self.nu.set_filter_gain(f, g)
            self.req[f] = (self.req.get(f, (None, None))[0], g)

    # ---- output gain: the header's ramp definition (nupc_chain_ref.GainRamp)
    def ramp(self, R):
        self.nu.set_gain_ramp(R)
        self.gr.set_ramp(R)

    def gain(self, ch, g):
        self.nu.set_output_gain(ch, g)
        self.gr.request(ch, g)

    def _commit_gain(self, b):
        self.gr.commit(b)

    def frames(self, raw):
        return nr.decode(raw, self.fmts, self.n)


def _check(got, want, rs):
    err = cases.rel_rms(got, want)
    print("rel rms %.3g" % err)
    assert err <= TOL[rs], err
    for b in range(0, len(want), L0):
        g, w = got[b:b + L0], want[b:b + L0]
        if np.abs(w).max() > 0:
            assert cases.rel_rms(g, w) <= TOL[rs], (b // L0, cases.rel_rms(g, w))
        else:
            assert np.all(g == 0), b // L0


def _bound(rig):
    for b, t, _, _ in rig.switches:
        assert b * L0 <= t <= b * L0 + MAX_OFF, (b, t)


def _check_ints(rig, raw):
    """integer outputs: within one count of the model's unrounded value, and the overflow count
    against the recount with the border allowance of test_s16_overflow_count_with_gain"""
    full = float(1 << (8 * rig.fmts[0].sbytes - 1))
    v = rig.blended() * rig.g * full + 0.5
    got = nr.ints(raw, rig.fmts, rig.n)
    d = np.abs(got - np.clip(np.floor(v), -full, full - 1))
    print("max count difference %d" % d.max())
    assert d.max() <= 1
    counts = []
    for ch in range(2):
        of = rig.nu.overflow(ch)
        recount = int(((v[:, ch] <= -full) | (v[:, ch] > full - 1)).sum())
        border = int((np.minimum(np.abs(v[:, ch] + full), np.abs(v[:, ch] - (full - 1))) < 1e-2 * full / 32768.0).sum())
        assert abs(int(of.n_overflows) - recount) <= border, (ch, of.n_overflows, recount)
        counts.append(recount)
    return counts


# ---------------------------------------------------------------- per-filter gain as part of a switch

@pytest.mark.parametrize("rs", [4, 8])
def test_gain_only_hard_switch_at_the_reported_frame(hip, rs):
    """F = 0; requests at blocks 5, 23 (not on the 512-frame grid) and 48 (on it: frame 3072); a
    negative gain, a zero and values above and below 1"""
    rig = Rig(hip, rs, 11 + rs, 80)
    acts = {5: lambda r: r.request(gains={0: -0.5, 1: 2.0, 2: 0.0, 3: 0.25}, F=0),
            23: lambda r: r.request(gains={0: 1.5, 2: -1.0}),
            48: lambda r: r.request(gains={f: 1.0 for f in range(4)})}
    got = rig.frames(rig.run(acts))
    assert [s[0] for s in rig.switches] == [5, 23, 48]
    assert rig.switches[1][3] == [(0, 1.5), (0, 2.0), (0, -1.0), (0, 0.25)]
    _bound(rig)
    _check(got, rig.blended(), rs)


@pytest.mark.parametrize("F", [2, 64, 200])
def test_gain_only_switch_with_crossfade(hip, F):
    """F = 200 is no multiple of L0 and spans periods"""
    rig = Rig(hip, 4, 23 + F, 70)
    acts = {7: lambda r: r.request(gains={0: 0.3, 1: -1.0, 3: 1.7}, F=F),
            40: lambda r: r.request(gains={0: 1.0, 2: 0.0})}
    got = rig.frames(rig.run(acts))
    assert [(s[0], s[2]) for s in rig.switches] == [(7, F), (40, F)]
    _bound(rig)
    _check(got, rig.blended(), 4)


def test_set_and_gain_changes_queued_together_are_one_switch(hip):
    rig = Rig(hip, 8, 31, 80, n_sets=2)
    frames_seen = []

    def after(r, b):
        frames_seen.append(r.nu.switch_frame())

    acts = {6: lambda r: r.request(sets={0: 1, 3: 1}, gains={0: 0.5, 1: -2.0}, F=100),
            45: lambda r: r.request(sets={0: 0}, gains={3: 0.75}, F=0)}
    got = rig.frames(rig.run(acts, after))
    assert [s[3] for s in rig.switches] == [[(1, 0.5), (0, -2.0), (0, 1.0), (1, 1.0)],
                                            [(0, 0.5), (0, -2.0), (0, 1.0), (1, 0.75)]]
    # switch_frame moved once per group
    moves = [b for b in range(1, 80) if frames_seen[b] != frames_seen[b - 1]]
    assert moves == [6, 45] and frames_seen[5] == -1
    _bound(rig)
    _check(got, rig.blended(), 8)


def test_both_filters_of_an_output_at_zero_give_exact_zeros(hip):
    rig = Rig(hip, 4, 41, 60)
    got = rig.frames(rig.run({4: lambda r: r.request(gains={2: 0.0, 3: 0.0}, F=64)}))
    (_, t, F, _), = rig.switches
    assert np.all(got[t + F:, 1] == 0) and np.any(got[t + F - 2, 1] != 0)
    _check(got, rig.blended(), 4)


def test_a_group_that_equals_the_live_gains_commits_nothing(hip):
    a = Rig(hip, 8, 51, 60, init_gain={1: 0.5})
    b = Rig(hip, 8, 51, 60, init_gain={1: 0.5})

    def same(r):
        r.nu.set_filter_gain(0, 1.0)
        r.nu.set_filter_gain(1, 0.5)

    ga, gb = a.run({9: same, 30: same}), b.run()
    assert a.switches == [] and a.nu.switch_frame() == -1 and not a.nu.switch_busy()
    assert np.array_equal(ga, gb)
    _check(a.frames(ga), a.blended(), 8)


def test_gain_state_and_argument_errors(hip):
    L = hip.lib()
    # before finalize: the initial gain, no reservation needed; shows from frame 0
    rig = Rig(hip, 4, 61, 70, init_gain={0: -0.5, 3: 0.0})
    nu, h = rig.nu, rig.nu.h
    assert L.bfhip_nupc_reserve_filter_gain(h) == ESTATE                       # after finalize
    assert [nu.get_filter_gain(f) for f in range(4)] == [-0.5, 1.0, 1.0, 0.0]
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.bfhip_nupc_set_filter_gain(h, 0, bad) == EINVAL
    assert L.bfhip_nupc_set_filter_gain(h, 4, 1.0) == EINVAL
    assert L.bfhip_nupc_set_filter_gain(h, -1, 1.0) == EINVAL
    assert np.isnan(L.bfhip_nupc_get_filter_gain(h, 4)) and np.isnan(L.bfhip_nupc_get_filter_gain(h, -1))
    for bad in (-1, 1048577):
        assert L.bfhip_nupc_set_gain_ramp(h, bad) == EINVAL
    assert L.bfhip_nupc_set_gain_ramp(h, 1048576) == 0 and L.bfhip_nupc_set_gain_ramp(h, 0) == 0
    seen = {}

    def after(r, b):
        if b == 5:
            seen["before"] = nu.get_filter_gain(1)                 # queued at block 6, not yet committed
        if b == 6:
            assert nu.switch_busy()
            seen["after"] = nu.get_filter_gain(1)
            seen["busy"] = (L.bfhip_nupc_set_filter_gain(h, 1, 3.0), L.bfhip_nupc_set_coeff(h, 1, 0))
        if b == 40:
            assert not nu.switch_busy()

    def ask(r):
        r.request(gains={1: 0.25})
        seen["queued"] = nu.get_filter_gain(1)

    got = rig.frames(rig.run({6: ask}, after))
    assert seen == {"before": 1.0, "queued": 1.0, "after": 0.25, "busy": (ESTATE, ESTATE)}
    assert [s[3] for s in rig.switches] == [[(0, -0.5), (0, 0.25), (0, 1.0), (0, 0.0)]]   # the refused call queued nothing
    assert nu.get_filter_gain(1) == 0.25
    _check(got, rig.blended(), 4)
    # without the reservation: ESTATE after finalize, even though a second set gives it the rings
    plain = Rig(hip, 4, 62, 4, n_sets=2, reserve=False)
    assert L.bfhip_nupc_set_filter_gain(plain.nu.h, 0, 0.5) == ESTATE
    assert plain.nu.get_filter_gain(0) == 1.0


# ---------------------------------------------------------------- ramped output gain

@pytest.mark.parametrize("rs,R", [(4, 1), (8, 48), (4, 64), (8, 150)])
def test_ramps_on_float_outputs(hip, rs, R):
    """g[t] as defined: a restart mid-ramp (block 21: the ramp of block 20 is R frames long), a
    same-target call mid-ramp (block 41), two channels with different phases, gains above and
    below 1, and a change of the ramp length that leaves a running ramp alone"""
    rig = Rig(hip, rs, 71 + R, 70)
    acts = {3: lambda r: (r.ramp(R), r.gain(0, 0.25)),
            9: lambda r: r.gain(1, 2.5),
            20: lambda r: (r.gain(0, 1.75), r.gain(1, 0.5)),
            21: lambda r: r.gain(0, 0.1),
            40: lambda r: (r.ramp(3 * R), r.gain(1, 3.0)),
            41: lambda r: (r.gain(1, 3.0), r.ramp(7)),
            55: lambda r: (r.gain(0, 0.5), r.gain(0, 1.0))}             # the last one counts
    got = rig.frames(rig.run(acts))
    if R > 64:
        assert rig.g[21 * L0 - 1, 0] not in (0.25, 1.75)                 # block 21 did restart a running ramp
        assert rig.g[41 * L0, 1] not in (0.5, 3.0)                       # block 41 came mid-ramp
    assert rig.g[-1, 0] == 1.0 and rig.g[-1, 1] == 3.0
    _check(got, rig.blended() * rig.g, rs)


@pytest.mark.parametrize("rs", [4, 8])
def test_ramp_zero_and_never_called_give_the_same_bits(hip, rs):
    """the step gains of test_output_gain_and_mute with set_gain_ramp(0) and without the call"""
    gains = {10: (0, 0.5), 20: (1, 0.0), 30: (1, 2.0), 33: (0, 1.0)}
    runs = []
    for call in (False, True):
        rig = Rig(hip, rs, 81, 60, out_gain={1: 0.5})
        acts = {b: (lambda r, c=c, g=g: r.gain(c, g)) for b, (c, g) in gains.items()}
        if call:
            acts[0] = lambda r: r.ramp(0)
        runs.append(rig.run(acts))
    assert np.array_equal(runs[0], runs[1])
    got = rig.frames(runs[1])
    assert np.all(got[20 * L0:30 * L0, 1] == 0)
    _check(got, rig.blended() * rig.g, rs)


@pytest.mark.parametrize("rs,outfmt", [(4, "S16_LE"), (8, "S24_4LE")])
def test_ramp_on_integer_outputs(hip, rs, outfmt):
    """no dither; the ramp to 40 clips part of channel 0.  The 24-bit output runs on the float64
    convolver: one count is 1.2e-7 of full scale, below the float32 convolver's own error against
    the float64 model (its bound is 1e-5 relative RMS), so "within one count of the model" can
    only be asked of float64 there; at 16 bits (3e-5 of full scale) float32 meets it."""
    rig = Rig(hip, rs, 91, 60, outfmt=outfmt)
    acts = {4: lambda r: (r.ramp(150), r.gain(0, 40.0)),
            12: lambda r: r.gain(1, 0.3),
            30: lambda r: (r.ramp(48), r.gain(0, 1.0))}
    raw = rig.run(acts)
    counts = _check_ints(rig, raw)
    assert counts[0] > 100 and counts[1] == 0


def test_ramp_to_zero_on_a_dithered_output_is_dithered_silence(hip):
    """from the first frame at gain 0 the bytes are the model's: the table walk went on"""
    rig = Rig(hip, 8, 101, 60, outfmt="S16_LE", dither=(0, 1))
    acts = {5: lambda r: (r.ramp(100), r.gain(0, 0.0)), 8: lambda r: r.gain(1, 0.0),
            40: lambda r: (r.ramp(64), r.gain(0, 1.0))}
    raw = rig.run(acts)
    want, _ = rig.want_raw()
    got, ref = nr.ints(raw, rig.fmts, rig.n), nr.ints(want, rig.fmts, rig.n)
    assert np.abs(got - ref).max() <= 1
    z0, z1 = 5 * L0 + 99, 8 * L0 + 99
    assert rig.g[z0, 0] == 0 and rig.g[z0 - 1, 0] != 0 and rig.g[z1, 1] == 0 and rig.g[z1 - 1, 1] != 0
    assert np.array_equal(got[z0:40 * L0, 0], ref[z0:40 * L0, 0])
    assert np.array_equal(got[z1:, 1], ref[z1:, 1])
    assert np.any(got[z0:40 * L0, 0] != 0) and np.abs(got[z0:40 * L0, 0]).max() <= 3


@pytest.mark.parametrize("rs", [4, 8])
def test_ramp_on_an_output_with_a_sub_sample_filter(hip, rs):
    """sdf_length 7: the FIR filters the ramped, scaled values"""
    rig = Rig(hip, rs, 111, 60, subdelay=7)
    acts = {3: lambda r: (r.ramp(150), r.gain(0, 0.2)), 5: lambda r: r.gain(1, 1.8),
            30: lambda r: (r.ramp(48), r.gain(0, 1.0), r.gain(1, 0.0))}
    raw = rig.run(acts)
    want, _ = rig.want_raw()
    _check(rig.frames(raw), rig.frames(want), rs)


def test_ramp_through_a_coefficient_switch_window(hip):
    """blend first, then gain"""
    rig = Rig(hip, 8, 121, 70, n_sets=2)
    acts = {5: lambda r: r.request(sets={f: 1 for f in range(4)}, gains={1: 0.5}, F=200),
            6: lambda r: (r.ramp(900), r.gain(0, 0.1), r.gain(1, 4.0))}
    got = rig.frames(rig.run(acts))
    (_, t, F, _), = rig.switches
    assert 6 * L0 < t + F < 6 * L0 + 900                                # the fade ends inside the ramp
    _check(got, rig.blended() * rig.g, 8)


def test_block_and_block_dev_same_bits(hip):
    """a script that mixes a gain-only switch, a cross-faded one, a set + gain group and ramps"""
    runs = []
    for dev in (False, True):
        rig = Rig(hip, 4, 131, 70, n_sets=2)
        acts = {4: lambda r: r.request(gains={0: -0.5, 2: 0.0}, F=0),
                9: lambda r: (r.ramp(150), r.gain(0, 0.25)),
                10: lambda r: r.gain(1, 2.0),
                30: lambda r: r.request(sets={1: 1}, gains={2: 1.5}, F=100),
                31: lambda r: (r.ramp(64), r.gain(0, 1.5))}
        runs.append(rig.run(acts, dev=dev))
    assert np.array_equal(runs[0], runs[1])
    assert len(rig.switches) == 2
    _check(rig.frames(runs[1]), rig.blended() * rig.g, 4)


# ---------------------------------------------------------------- peak reset

def test_reset_overflow(hip):
    """a clipped stretch, then a reset in front of block 30: the structs equal the model's started
    afresh at that block; the status bits of the call are unaffected"""
    rig = Rig(hip, 8, 141, 60, outfmt="S16_LE", amp=0.2)
    assert hip.lib().bfhip_nupc_set_safety_limit(rig.nu.h, 30.0) == 0
    before = {}

    def reset(r):
        before["of"] = [r.nu.overflow(c) for c in range(2)]
        r.nu.reset_overflow()

    acts = {3: lambda r: r.gain(0, 20.0), 20: lambda r: r.gain(0, 1.0), 30: reset,
            45: lambda r: r.gain(1, 15.0)}
    rig.run(acts)
    assert before["of"][0].n_overflows > 50 and before["of"][0].largest > 32767.0
    _, want = rig.want_raw(first_block=30)
    for c in range(2):
        of, w = rig.nu.overflow(c), want[c]
        assert (of.n_overflows, of.intlargest, of.max) == (w.n_overflows, w.intlargest, w.max), c
        assert of.largest == pytest.approx(w.largest, rel=1e-9)
    assert rig.nu.overflow(0).n_overflows == 0 and rig.nu.overflow(1).n_overflows > 0
    # the status bits: a sample over the safety limit is reported by the call a reset precedes
    nu = rig.nu
    nu.set_output_gain(0, 2000.0)
    nu.reset_overflow()
    st, _ = nu.block(rig.x[:L0])
    assert st == hip.ST_SAFETY
    assert hip.lib().bfhip_nupc_reset_overflow(nu.h) == 0
    of = nu.overflow(0)
    assert (of.n_overflows, of.intlargest, of.largest, of.max) == (0, 0, 0.0, 32767.0)
