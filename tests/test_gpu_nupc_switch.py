"""GPU: run-time control of the non-uniform convolver (include/bfhip_nupc.h): coefficient switches
with and without cross-fade, presets, set rewrites and output gain.  Reference: float64 numpy
convolutions of the whole input under each assignment, blended by the header's definition at
the switch frame the library reports (float32 1e-5 / float64 1e-12 relative RMS, over the whole
run and per 64-frame block).  Every impulse response is flat noise over the whole schedule, and
the sets of a filter differ in every segment: a switch applied to one segment at the wrong frame
shows."""
import ctypes as C

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])     # offsets 0, 128, 384, 896
EINVAL, ESTATE = -1, -5


def _conv(x, h, n):
    m = len(x) + len(h) - 1
    nfft = 1 << (m - 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x, nfft) * np.fft.rfft(h, nfft), nfft)[:n]


class Rig:
    """a 2x2 crossbar (filter f = 2 * out + in) with n_sets impulse responses per filter"""

    def __init__(self, hip, rs, n_sets, seed, sched=SMALL, outfmt=None, ref_taps=None, n_frames=0, add_sets=None):
        self.rs, self.dt = rs, (np.float32 if rs == 4 else np.float64)
        self.nu = nu = hip.Nupc(sched[0], sched[1], rs, 2, 2)
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, outfmt or FF[rs])
        rng = np.random.default_rng(seed)
        self.h = [[(rng.standard_normal(nu.taps) / np.sqrt(nu.taps)).astype(self.dt) for _ in range(n_sets)]
                  for _ in range(4)]
        self.scales = [(0.5 if f % 2 else 1.0) * (-1.0 if f // 2 else 1.0) for f in range(4)]
        for f in range(4):
            nu.add_filter(f % 2, f // 2, self.h[f][0], in_scale=0.5 if f % 2 else 1.0,
                          out_scale=-1.0 if f // 2 else 1.0)
            for j in range(1, n_sets if add_sets is None else add_sets):
                assert nu.add_coeff(f, self.h[f][j]) == j
        nu.finalize()
        self.L0 = nu.L0
        self.ref_taps = ref_taps or nu.taps
        self.x = (rng.standard_normal((n_frames, 2)) * 0.1).astype(self.dt)
        self._y = {}

    def y(self, asg):
        """full-history float64 output under an assignment (filter -> set)"""
        n = len(self.x)
        out = np.zeros((n, 2))
        for f in range(4):
            key = (f, asg[f])
            if key not in self._y:
                h = self.h[f][asg[f]][:self.ref_taps].astype(np.float64)
                self._y[key] = _conv(self.x[:, f % 2].astype(np.float64), h, n) * self.scales[f]
            out[:, f // 2] += self._y[key]
        return out

    def run(self, actions=None, after=None):
        """block by block; actions[b](rig) runs before block call b.  Returns the output and the
        committed switches [(block, t_sw, F, assignment)]"""
        nu, L0 = self.nu, self.L0
        self.asg, self.req, self.F, self.switches = [0] * 4, {}, L0, []
        got, t_last = [], nu.switch_frame()
        assert t_last == -1
        for b in range(len(self.x) // L0):
            if actions and b in actions:
                actions[b](self)
            st, raw = nu.block(self.x[b * L0:(b + 1) * L0])
            assert st == 0
            got.append(raw)
            t = nu.switch_frame()
            if t != t_last:
                new = list(self.asg)
                for f, c in self.req.items():
                    new[f] = c
                self.switches.append((b, t, self.F, new))
                self.asg, self.req, t_last = new, {}, t
            if after:
                after(self, b)
        return np.concatenate(got)

    def request(self, changes, F=None):
        if F is not None:
            self.F = F
            self.nu.set_crossfade(F)
        assert not self.nu.switch_busy()
        for f, c in changes.items():
            self.nu.set_coeff(f, c)
            self.req[f] = c

    def want(self):
        out = self.y([0] * 4)
        prev = [0] * 4
        n = len(out)
        for _, t, F, asg in self.switches:
            yo, yn = self.y(prev), self.y(asg)
            out[t:] = yn[t:]
            if F:
                j = np.arange(min(F, n - t))
                w = (j / (F - 1))[:, None]
                out[t:t + len(j)] = (1 - w) * yo[t:t + len(j)] + w * yn[t:t + len(j)]
            prev = asg
        return out


def _frames(raw, dt):
    return np.frombuffer(raw.tobytes(), dt).reshape(-1, 2).astype(np.float64)


def _check(got, want, rs, L0=64):
    assert cases.rel_rms(got, want) <= TOL[rs]
    for b in range(0, len(want), L0):
        if np.abs(want[b:b + L0]).max() > 0:
            assert cases.rel_rms(got[b:b + L0], want[b:b + L0]) <= TOL[rs], b // L0


def _bound(rig):
    max_off = sum(a * b for a, b in zip(SMALL[0][:-1], SMALL[1][:-1]))
    for b, t, _, _ in rig.switches:
        t_req = b * rig.L0
        assert t_req <= t <= t_req + max_off, (b, t)


@pytest.mark.parametrize("rs", [4, 8])
def test_hard_switch_at_the_reported_frame(hip, rs):
    """F = 0; requests at blocks 5, 37, 83 (not on the 512-frame grid) and 120 (on it)"""
    rig = Rig(hip, rs, 2, 11 + rs, n_frames=64 * 160)
    acts = {b: (lambda r, c=c: r.request({f: c for f in range(4)}, F=0))
            for b, c in ((5, 1), (37, 0), (83, 1), (120, 0))}
    got = _frames(rig.run(acts), rig.dt)
    assert [s[0] for s in rig.switches] == [5, 37, 83, 120]
    _bound(rig)
    _check(got, rig.want(), rs)


@pytest.mark.parametrize("F", [64, 5 * 64 + 3])
def test_crossfade(hip, F):
    rig = Rig(hip, 4, 2, 23, n_frames=64 * 140)
    acts = {7: lambda r: r.request({f: 1 for f in range(4)}, F=F),
            70: lambda r: r.request({f: 0 for f in range(4)})}
    got = _frames(rig.run(acts), rig.dt)
    assert len(rig.switches) == 2
    _bound(rig)
    _check(got, rig.want(), 4)


def test_preset_and_back(hip):
    """several filters in one call group, the rest unchanged; A -> B -> A -> C"""
    rig = Rig(hip, 8, 3, 31, n_frames=64 * 150)
    acts = {4: lambda r: r.request({0: 1, 3: 2}),
            45: lambda r: r.request({0: 0, 3: 0}, F=200),
            90: lambda r: r.request({1: 2, 2: 1, 3: 1}, F=0)}
    got = _frames(rig.run(acts), rig.dt)
    assert [s[3] for s in rig.switches] == [[1, 0, 0, 2], [0, 0, 0, 0], [0, 2, 1, 1]]
    _bound(rig)
    _check(got, rig.want(), 8)


def test_state_and_argument_errors(hip):
    L = hip.lib()
    rig = Rig(hip, 4, 2, 41, n_frames=64 * 90)
    h = rig.nu.h
    taps = np.zeros(16, np.float32)
    assert L.bfhip_nupc_add_coeff(h, 0, taps.ctypes.data_as(C.c_void_p), 16) == ESTATE     # after finalize
    assert L.bfhip_nupc_set_crossfade(h, 1) == EINVAL
    assert L.bfhip_nupc_set_crossfade(h, 1048577) == EINVAL
    assert L.bfhip_nupc_set_crossfade(h, -3) == EINVAL
    assert L.bfhip_nupc_set_coeff(h, 4, 0) == EINVAL
    assert L.bfhip_nupc_set_coeff(h, 0, 2) == EINVAL
    assert L.bfhip_nupc_set_coeff(h, 0, -1) == EINVAL
    assert L.bfhip_nupc_set_output_gain(h, 2, 1.0) == EINVAL
    assert rig.nu.switch_busy() is False and rig.nu.switch_frame() == -1
    refused = []

    def after(r, b):
        if b == 6:
            assert r.nu.switch_busy()
            # refused while the switch is in flight, and nothing is queued by it
            refused.append(L.bfhip_nupc_set_coeff(h, 0, 0))
        if b == 40:
            assert not r.nu.switch_busy()

    acts = {6: lambda r: r.request({f: 1 for f in range(4)}),
            45: lambda r: r.request({0: 0})}
    got = _frames(rig.run(acts, after), rig.dt)
    assert refused == [ESTATE]
    assert [s[0] for s in rig.switches] == [6, 45]
    assert rig.switches[1][3] == [0, 1, 1, 1]
    _check(got, rig.want(), 4)


def test_set_before_finalize_is_refused(hip):
    nu = hip.Nupc(*SMALL, 4, 1, 1)
    nu.add_filter(0, 0, np.ones(8, np.float32))
    assert nu.add_coeff(0, np.ones(8, np.float32)) == 1
    assert hip.lib().bfhip_nupc_set_coeff(nu.h, 0, 1) == ESTATE
    with pytest.raises(hip.BfhipError):
        nu.add_coeff(0, np.ones(nu.taps + 1, np.float32))


def test_update_idle_set_then_switch(hip):
    L = hip.lib()
    rig = Rig(hip, 8, 3, 51, n_frames=64 * 110)
    nu = rig.nu
    fresh = (np.random.default_rng(99).standard_normal(nu.taps) / np.sqrt(nu.taps)).astype(np.float64)
    p = fresh.ctypes.data_as(C.c_void_p)
    seen = []

    def upd(r):
        assert L.bfhip_nupc_update_coeff(nu.h, 1, 0, p, nu.taps) == ESTATE      # live
        r.request({1: 1})
        assert L.bfhip_nupc_update_coeff(nu.h, 1, 1, p, nu.taps) == ESTATE      # queued
        nu.update_coeff(1, 2, fresh)                                             # idle
        r.h[1][2] = fresh

    def after(r, b):
        if b == 10:
            assert nu.switch_busy()
            seen.append(L.bfhip_nupc_update_coeff(nu.h, 1, 0, p, nu.taps))      # old side of the window
            seen.append(L.bfhip_nupc_update_coeff(nu.h, 1, 1, p, nu.taps))      # new side

    acts = {3: upd, 60: lambda r: r.request({1: 2}, F=0)}
    got = _frames(rig.run(acts, after), rig.dt)
    assert seen == [ESTATE, ESTATE]
    assert [s[3] for s in rig.switches] == [[0, 1, 0, 0], [0, 2, 0, 0]]
    _check(got, rig.want(), 8)


def test_output_gain_and_mute(hip):
    rig = Rig(hip, 4, 2, 61, n_frames=64 * 80)
    gains = {10: (0, 0.5), 20: (1, 0.0), 30: (1, 2.0), 33: (0, 1.0)}
    acts = {b: (lambda r, c=c, g=g: r.nu.set_output_gain(c, g)) for b, (c, g) in gains.items()}
    acts[25] = lambda r: r.request({f: 1 for f in range(4)})
    got = _frames(rig.run(acts), rig.dt)
    want = rig.want()
    g = np.ones_like(want)
    for b, (c, v) in sorted(gains.items()):
        g[b * 64:, c] = v
    want *= g
    assert np.all(got[20 * 64:30 * 64, 1] == 0)
    _check(got[:20 * 64], want[:20 * 64], 4)
    _check(got[:, 0], want[:, 0], 4)
    _check(got[30 * 64:], want[30 * 64:], 4)


def test_s16_overflow_count_with_gain(hip):
    rig = Rig(hip, 4, 2, 71, outfmt="S16_LE", n_frames=64 * 60)
    acts = {5: lambda r: r.nu.set_output_gain(0, 1000.0), 12: lambda r: r.request({f: 1 for f in range(4)})}
    raw = rig.run(acts)
    want = rig.want()
    want[5 * 64:, 0] *= 1000.0
    v = want * 32768.0 + 0.5
    for ch in range(2):
        of = rig.nu.overflow(ch)
        recount = int(((v[:, ch] <= -32768.0) | (v[:, ch] > 32767.0)).sum())
        border = int((np.minimum(np.abs(v[:, ch] + 32768.0), np.abs(v[:, ch] - 32767.0)) < 1e-2).sum())
        assert abs(int(of.n_overflows) - recount) <= border, (ch, of.n_overflows, recount)
        if ch == 0:
            assert recount > 100
    got = np.frombuffer(raw.tobytes(), np.int16).reshape(-1, 2).astype(np.float64)
    clipped = np.clip(np.floor(v), -32768, 32767)
    assert np.abs(got - clipped).max() <= 1


def test_room_correction_switch_float64(hip):
    """BASELINE configs[4]: 1 M taps, float64, 64-frame latency, one mid-run switch, 6 x 8192
    frames; the reference truncates the impulse responses to the frames run"""
    seg_len, k = [], 64
    while k < 8192:
        seg_len.append(k)
        k *= 2
    covered = 2 * sum(seg_len)
    sched = (seg_len + [8192], [2] * len(seg_len) + [-(-(1048576 - covered) // 8192)])
    n = 6 * 8192
    rig = Rig(hip, 8, 2, 81, sched=sched, ref_taps=n, n_frames=n)
    got = _frames(rig.run({300: lambda r: r.request({f: 1 for f in range(4)})}), rig.dt)
    (b, t, _, _), = rig.switches
    assert 300 * 64 <= t <= 300 * 64 + covered
    _check(got, rig.want(), 8)


def test_block_and_block_dev_same_bits(hip):
    import torch
    runs = []
    for dev in (False, True):
        rig = Rig(hip, 4, 2, 91, n_frames=64 * 70)
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
            if b == 15:
                nu.set_output_gain(1, 0.25)
            xb = rig.x[b * 64:(b + 1) * 64]
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
        runs.append(np.concatenate(out))
    assert np.array_equal(runs[0], runs[1])


def test_unused_sets_change_nothing(hip):
    a = Rig(hip, 8, 3, 101, n_frames=64 * 40)
    b = Rig(hip, 8, 3, 101, n_frames=64 * 40, add_sets=1)
    ga, gb = a.run(), b.run()
    assert np.array_equal(ga, gb)
    _check(_frames(ga, np.float64), a.want(), 8)
