"""GPU: set rewrites of the non-uniform convolver that never stall the audio thread
(bfhip_nupc_reserve_update / _update_coeff_async / _update_coeff_dev_async / _update_busy /
_update_result / _update_wait, include/bfhip_nupc.h).

What must hold: the asynchronous rewrite prepares a set with the arithmetic of the synchronous
bfhip_nupc_update_coeff, so a run that switches onto the rewritten set has the same BYTES under
both; a rewrite of an idle set changes no output byte; and the output after the switch is the
float64 model's (tests/nupc_ref.py: plain float64 convolutions blended at the reported switch
frame; float32 1e-5 / float64 1e-12 relative RMS over the whole run and per block, the tolerances
of tests/test_gpu_nupc_switch.py).

Schedule S = 64, 128, 256, 512 x 2, 2, 2, 6: the LDS transform, main and background streams.
Schedule B = 4096, 8192, 16384 x 2, 2, 2: the wave transform and the big-FFT sequence with its
shared scratch.  A 2x2 crossbar, three sets per filter of flat noise over the whole schedule: a
slice prepared for the wrong segment or offset shows."""
import ctypes as C

import numpy as np
import pytest

import cases
import nupc_ref

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
FF = {4: "FLOAT_LE", 8: "FLOAT64_LE"}
SCHED = {"S": ([64, 128, 256, 512], [2, 2, 2, 6]), "B": ([4096, 8192, 16384], [2, 2, 2])}
# blocks run, block the rewrite starts before, block the switch is requested before
PLAN = {"S": (110, 3, 40), "B": (24, 1, 10)}
EINVAL, ESTATE = -1, -5
NAN_MSG = b"NaN or Inf value among coefficients."


def _noise(seed, n, dt):
    return (np.random.default_rng(seed).standard_normal(n) / np.sqrt(n)).astype(dt)


class Rig:
    """a 2x2 crossbar (filter f = 2 * out + in), three sets per filter, update reservation"""

    def __init__(self, hip, rs, sched, seed, n_blocks, reserve=True):
        self.hip, self.rs, self.dt = hip, rs, (np.float32 if rs == 4 else np.float64)
        self.nu = nu = hip.Nupc(sched[0], sched[1], rs, 2, 2)
        nu.set_interleaved(0, FF[rs])
        nu.set_interleaved(1, FF[rs])
        if reserve:
            nu.reserve_update()
        self.h = [[_noise(1000 * seed + 10 * f + j, nu.taps, self.dt) for j in range(3)] for f in range(4)]
        self.scales = [(0.5 if f % 2 else 1.0) * (-1.0 if f // 2 else 1.0) for f in range(4)]
        for f in range(4):
            nu.add_filter(f % 2, f // 2, self.h[f][0], in_scale=0.5 if f % 2 else 1.0, out_scale=-1.0 if f // 2 else 1.0)
            for j in (1, 2):
                assert nu.add_coeff(f, self.h[f][j]) == j
        nu.finalize()
        self.L0 = nu.L0
        self.x = (np.random.default_rng(seed).standard_normal((n_blocks * nu.L0, 2)) * 0.1).astype(self.dt)
        self.asg, self.req, self.F = [0] * 4, {}, nu.L0
        self.ys, self.switches = [], []           # model: outputs per assignment, [(t_sw, F, index)]
        self.idle_at = None

    def y(self):
        """float64 output under the sets as they are now and the assignment in force"""
        filters = [(f % 2, f // 2, self.h[f][self.asg[f]], 1.0, self.scales[f]) for f in range(4)]
        return nupc_ref.convolve(self.x.astype(np.float64), filters, 2)

    def request(self, changes, F=None):
        if F is not None:
            self.F = F
            self.nu.set_crossfade(F)
        for f, c in changes.items():
            self.nu.set_coeff(f, c)
            self.req[f] = c

    def run(self, actions=None, after=None):
        """block by block; actions[b](rig) runs before block call b, after(rig, b) behind it"""
        nu, L0 = self.nu, self.L0
        self.ys = [self.y()]
        got, t_last = [], nu.switch_frame()
        for b in range(len(self.x) // L0):
            if actions and b in actions:
                actions[b](self)
            st, raw = nu.block(self.x[b * L0:(b + 1) * L0])
            assert st == 0
            got.append(raw)
            t = nu.switch_frame()
            if t != t_last:
                for f, c in self.req.items():
                    self.asg[f] = c
                self.req, t_last = {}, t
                self.ys.append(self.y())
                self.switches.append((t, self.F, len(self.ys) - 1))
            if self.idle_at is None and not nu.update_busy():
                self.idle_at = b
            if after:
                after(self, b)
        return np.concatenate(got)

    def want(self):
        return nupc_ref.switched(self.ys, self.switches)

    # the two ways to rewrite: set j of the listed filters, one after the other
    def rewrite_sync(self, sets, new):
        for (f, j), h in zip(sets, new):
            self.nu.update_coeff(f, j, h)
            self.h[f][j] = np.concatenate([h, np.zeros(self.nu.taps - len(h), self.dt)])

    def rewrite_async(self, sets, new, how="host"):
        """starts the first rewrite now; returns the `after` hook that starts the next as busy clears
        (one poll per block call)"""
        todo = list(zip(sets, new))
        self.idle_at = None
        self.keep = []

        def start():
            (f, j), h = todo.pop(0)
            if how == "buffer":                    # render in place, pass the staging buffer itself
                buf = self.nu.update_buffer()
                buf[:len(h)] = h
                self.nu.update_coeff_async(f, j, buf[:len(h)])
            elif how == "device":
                import torch
                t = torch.from_numpy(np.ascontiguousarray(h)).cuda()
                ev = torch.cuda.Event()
                ev.record()
                self.keep.append((t, ev))          # the caller's buffer until busy is 0
                self.nu.update_coeff_dev_async(f, j, t, len(h), ev.cuda_event)
            else:
                self.nu.update_coeff_async(f, j, h)
            self.h[f][j] = np.concatenate([h, np.zeros(self.nu.taps - len(h), self.dt)])

        def after(rig, b):
            if todo and not self.nu.update_busy():
                assert self.nu.update_result() == 0
                self.idle_at = None
                start()

        start()
        return after


def _frames(raw, dt):
    return np.frombuffer(raw.tobytes(), dt).reshape(-1, 2).astype(np.float64)


def _check(got, want, rs, L0):
    print("rel rms whole run %.3g (limit %g)" % (cases.rel_rms(got, want), TOL[rs]))
    assert cases.rel_rms(got, want) <= TOL[rs]
    for b in range(0, len(want), L0):
        if np.abs(want[b:b + L0]).max() > 0:
            assert cases.rel_rms(got[b:b + L0], want[b:b + L0]) <= TOL[rs], b // L0


def _switch_run(hip, rs, key, mode, seed=7, how="host", n_taps=None):
    """rewrite set 2 of filters 0 and 3 before block b (sync or async), switch 0 -> 2, 3 -> 2, 1 -> 1
    before block s.  Returns (rig, raw output)"""
    n_blocks, b0, s = PLAN[key]
    rig = Rig(hip, rs, SCHED[key], seed, n_blocks)
    n_taps = n_taps or rig.nu.taps
    new = [_noise(5000 + seed, rig.nu.taps, rig.dt)[:n_taps], _noise(6000 + seed, rig.nu.taps, rig.dt)[:n_taps]]
    sets = [(0, 2), (3, 2)]
    hook = {}

    def rewrite(r):
        if mode == "sync":
            r.rewrite_sync(sets, new)
        else:
            hook["after"] = r.rewrite_async(sets, new, how)

    def switch(r):
        if mode != "sync":
            assert not r.nu.update_busy(), "the rewrites were still in flight at block %d" % s
            assert r.nu.update_result() == 0
            assert r.idle_at is not None and r.idle_at < s
        r.request({0: 2, 3: 2, 1: 1})

    raw = rig.run({b0: rewrite, s: switch}, lambda r, b: hook["after"](r, b) if "after" in hook else None)
    assert len(rig.switches) == 1
    return rig, raw


# ---------------------------------------------------------------- 1: same bits as the synchronous rewrite

@pytest.mark.parametrize("key", ["S", "B"])
@pytest.mark.parametrize("rs", [4, 8])
def test_async_rewrite_has_the_bits_of_the_synchronous_one(hip, rs, key):
    a, raw_a = _switch_run(hip, rs, key, "sync")
    b, raw_b = _switch_run(hip, rs, key, "async")
    assert a.nu.switch_frame() == b.nu.switch_frame() and a.switches == b.switches
    assert np.array_equal(raw_a, raw_b)
    _check(_frames(raw_b, b.dt), b.want(), rs, b.L0)


# ---------------------------------------------------------------- 2: an idle rewrite disturbs nothing

@pytest.mark.parametrize("key", ["S", "B"])
def test_idle_rewrite_changes_no_byte(hip, key):
    n_blocks, b0, _ = PLAN[key]
    runs = []
    for rewrite in (True, False):
        rig = Rig(hip, 4, SCHED[key], 17, n_blocks)
        hook = {}
        acts = {}
        if rewrite:
            new = [_noise(5100 + f, rig.nu.taps, rig.dt) for f in range(4)]
            acts[b0] = lambda r: hook.update(after=r.rewrite_async([(f, 2) for f in range(4)], new))
        # a switch between the other two sets while the rewrites are running
        acts[b0 + 2] = lambda r: r.request({f: 1 for f in range(4)})
        runs.append(rig.run(acts, lambda r, b: hook["after"](r, b) if "after" in hook else None))
        if rewrite:
            assert rig.nu.update_wait() == 0
    assert np.array_equal(runs[0], runs[1])


# ---------------------------------------------------------------- 3: switch back onto a rewritten set

# blocks before which: 0 -> 1 is requested, set 0 is rewritten (the window has closed), 1 -> 0 is requested
BACK = {"S": (3, 45, 70), "B": (1, 10, 15)}


@pytest.mark.parametrize("key,stream_copy", [("S", False), ("S", True), ("B", False)])
def test_switch_back_onto_a_rewritten_set(hip, key, stream_copy, monkeypatch):
    """0 -> 1, window closed, set 0 rewritten in place, 1 -> 0: the new taps play, not the old ones a
    layout keyed by the set's address could still hold (BFHIP_COEFF_STREAM=2 forces the segment
    engines' stream-ordered copy, which is such a layout)"""
    if stream_copy:
        monkeypatch.setenv("BFHIP_COEFF_STREAM", "2")
    n_blocks = PLAN[key][0]
    b0, mid, last = BACK[key]
    outs = []
    for mode in ("async", "sync"):
        rig = Rig(hip, 4, SCHED[key], 27, n_blocks)
        new = [_noise(5200 + f, rig.nu.taps, rig.dt) for f in (0, 3)]
        sets = [(0, 0), (3, 0)]
        hook = {}

        def rewrite(r):
            assert not r.nu.switch_busy()
            if mode == "sync":
                r.rewrite_sync(sets, new)
            else:
                hook["after"] = r.rewrite_async(sets, new)

        def back(r):
            if mode == "async":
                assert r.nu.update_wait() == 0
            assert all(np.array_equal(r.h[f][0], h) for (f, _), h in zip(sets, new))     # both were started
            r.request({f: 0 for f in range(4)})

        raw = rig.run({b0: lambda r: r.request({f: 1 for f in range(4)}), mid: rewrite, last: back},
                      lambda r, b: hook["after"](r, b) if "after" in hook else None)
        assert len(rig.switches) == 2
        got, want = _frames(raw, rig.dt), rig.want()
        _check(got, want, 4, rig.L0)
        t = rig.switches[1][0] + rig.L0
        assert t < len(want) - rig.L0 and cases.rel_rms(got[t:], want[t:]) <= TOL[4]
        outs.append(raw)
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------- 4: rewrite during a switch window

@pytest.mark.parametrize("key", ["S", "B"])
def test_rewrite_inside_a_switch_window(hip, key):
    n_blocks, b0, s = PLAN[key]
    rig = Rig(hip, 8, SCHED[key], 37, n_blocks)
    new = [_noise(5300 + f, rig.nu.taps, rig.dt) for f in range(4)]
    hook = {}
    F = 3 * rig.L0 + 5

    def rewrite(r):
        assert r.nu.switch_busy()                  # dual blocks are running
        L = hip.lib()
        p = new[0].ctypes.data_as(C.c_void_p)
        assert L.bfhip_nupc_update_coeff_async(r.nu.h, 0, 0, p, r.nu.taps) == ESTATE     # old side of the window
        assert L.bfhip_nupc_update_coeff_async(r.nu.h, 0, 1, p, r.nu.taps) == ESTATE     # new side
        hook["after"] = r.rewrite_async([(f, 2) for f in range(4)], new)

    def to2(r):
        assert not r.nu.switch_busy() and not r.nu.update_busy() and r.nu.update_result() == 0
        r.request({f: 2 for f in range(4)})

    raw = rig.run({b0: lambda r: r.request({f: 1 for f in range(4)}, F=F), b0 + 1: rewrite, s + (2 if key == "B" else 0): to2},
                  lambda r, b: hook["after"](r, b) if "after" in hook else None)
    assert len(rig.switches) == 2
    _check(_frames(raw, rig.dt), rig.want(), 8, rig.L0)


# ---------------------------------------------------------------- 5: zero-copy and padding

@pytest.mark.parametrize("key,n_taps", [("S", 0), ("S", 700), ("B", 20000)])
def test_staging_buffer_in_place_and_zero_padding(hip, key, n_taps):
    """the staging buffer filled in place and passed itself, against a separate array; n_taps 700 /
    20000 end inside a partition of the third segment: what the set held past them is gone"""
    a, raw_a = _switch_run(hip, 4, key, "async", how="host", n_taps=n_taps or None)
    b, raw_b = _switch_run(hip, 4, key, "async", how="buffer", n_taps=n_taps or None)
    assert np.array_equal(raw_a, raw_b)
    _check(_frames(raw_b, b.dt), b.want(), 4, b.L0)


def test_a_short_rewrite_leaves_nothing_of_a_longer_one(hip):
    n_blocks, b0, s = PLAN["S"]
    rig = Rig(hip, 8, SCHED["S"], 47, n_blocks)
    full, short = _noise(5400, rig.nu.taps, rig.dt), _noise(5401, rig.nu.taps, rig.dt)[:333]
    hook = {}
    acts = {b0: lambda r: hook.update(after=r.rewrite_async([(2, 2), (2, 2)], [full, short], "buffer")),
            s: lambda r: (r.nu.update_wait(), r.request({2: 2}))}
    raw = rig.run(acts, lambda r, b: hook["after"](r, b) if "after" in hook else None)
    assert not np.any(rig.h[2][2][333:]) and len(rig.switches) == 1
    _check(_frames(raw, rig.dt), rig.want(), 8, rig.L0)


# ---------------------------------------------------------------- 6: device source

@pytest.mark.parametrize("key", ["S", "B"])
def test_device_source_has_the_bits_of_the_host_source(hip, key):
    a, raw_a = _switch_run(hip, 4, key, "async", how="host")
    b, raw_b = _switch_run(hip, 4, key, "async", how="device")
    assert np.array_equal(raw_a, raw_b)


# ---------------------------------------------------------------- 7: block_dev with periods in flight

def test_block_dev_with_periods_in_flight(hip):
    import torch
    K, n_blocks = 12, 60
    outs = []
    for dev in (True, False):
        rig = Rig(hip, 4, SCHED["S"], 57, n_blocks)
        nu, L0 = rig.nu, rig.L0
        new = _noise(5500, nu.taps, rig.dt)
        raw_in = np.ascontiguousarray(rig.x).view(np.uint8).reshape(n_blocks, -1)
        if dev:
            din = torch.from_numpy(raw_in.copy()).cuda()
            dout = torch.zeros((n_blocks, nu.out_bytes), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
        out = []
        for b in range(n_blocks):
            if b == 3:
                nu.update_coeff_async(1, 2, new)
            if b == 3 + K:
                if dev:
                    assert nu.sync() == 0
                assert nu.update_wait() == 0
                nu.set_coeff(1, 2)
            if dev:
                nu.block_dev(din[b], dout[b])      # no host wait between the calls
            else:
                st, raw = nu.block(raw_in[b])
                assert st == 0
                out.append(raw)
        if dev:
            assert nu.sync() == 0
            out = [dout.cpu().numpy().ravel()]
        outs.append(np.concatenate(out))
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------- 8: states and errors

def test_argument_and_state_errors(hip):
    import torch
    L = hip.lib()
    rig = Rig(hip, 4, SCHED["S"], 67, 8)
    nu, h = rig.nu, rig.nu.h
    taps = _noise(5600, nu.taps, rig.dt)
    p = taps.ctypes.data_as(C.c_void_p)
    buf = nu.update_buffer()
    assert buf is not None and buf.shape == (nu.taps,) and buf.dtype == rig.dt
    assert L.bfhip_nupc_reserve_update(h) == ESTATE                              # after finalize
    for call in (lambda f, c, q, n: L.bfhip_nupc_update_coeff_async(h, f, c, q, n),
                 lambda f, c, q, n: L.bfhip_nupc_update_coeff_dev_async(h, f, c, q, n, None)):
        assert call(4, 2, p, nu.taps) == EINVAL
        assert call(-1, 2, p, nu.taps) == EINVAL
        assert call(0, 3, p, nu.taps) == EINVAL
        assert call(0, 2, None, nu.taps) == EINVAL
        assert call(0, 2, p, 0) == EINVAL
        assert call(0, 2, p, nu.taps + 1) == EINVAL
        assert call(0, 0, p, nu.taps) == ESTATE                                  # live
    assert not nu.update_busy()

    # busy: a device source whose ready event sits behind a long job on another stream
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    t = torch.from_numpy(taps).cuda()
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(side):
        for _ in range(40):
            a = (a @ a) * 1e-3
        ev.record(side)
    nu.update_coeff_dev_async(2, 2, t, nu.taps, ev.cuda_event)
    assert nu.update_busy()
    assert L.bfhip_nupc_update_coeff_async(h, 3, 2, p, nu.taps) == ESTATE
    assert L.bfhip_nupc_update_coeff_dev_async(h, 3, 2, C.c_void_p(t.data_ptr()), nu.taps, None) == ESTATE
    assert L.bfhip_nupc_update_coeff(h, 3, 2, p, nu.taps) == ESTATE
    assert b"in flight" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_update_result(h) == ESTATE
    assert L.bfhip_nupc_set_coeff(h, 2, 2) == ESTATE                             # the set being rewritten
    assert nu.update_wait() == 0 and not nu.update_busy() and nu.update_result() == 0
    nu.set_coeff(2, 2)
    assert L.bfhip_nupc_update_coeff_async(h, 2, 2, p, nu.taps) == ESTATE        # queued
    assert nu.block(rig.x[:64])[0] == 0
    assert nu.switch_busy()
    assert L.bfhip_nupc_update_coeff_async(h, 2, 0, p, nu.taps) == ESTATE        # old side of the window
    assert L.bfhip_nupc_update_coeff_async(h, 2, 2, p, nu.taps) == ESTATE        # new side
    nu.update_coeff_async(2, 1, taps)                                            # idle
    assert nu.update_wait() == 0


def test_set_0_keeps_add_filter_length(hip):
    L = hip.lib()
    nu = hip.Nupc(*SCHED["S"], 4, 1, 1)
    nu.reserve_update()
    nu.add_filter(0, 0, _noise(1, 300, np.float32))           # segments 0 and 1, and 44 taps of segment 2
    assert nu.add_coeff(0, _noise(2, nu.taps, np.float32)) == 1
    nu.finalize()
    nu.set_coeff(0, 1)
    x = np.zeros((64, 1), np.float32)
    for _ in range(40):
        nu.block(x)
    assert not nu.switch_busy()
    long = _noise(3, nu.taps, np.float32)
    assert L.bfhip_nupc_update_coeff_async(nu.h, 0, 0, long.ctypes.data_as(C.c_void_p), nu.taps) == EINVAL
    padded = long.copy()
    padded[640:] = 0                                           # set 0 has one 256-partition: taps [384, 640)
    nu.update_coeff_async(0, 0, padded)
    assert nu.update_wait() == 0
    import torch
    t = torch.from_numpy(padded).cuda()
    torch.cuda.synchronize()
    assert L.bfhip_nupc_update_coeff_dev_async(nu.h, 0, 0, C.c_void_p(t.data_ptr()), nu.taps, None) == EINVAL
    nu.update_coeff_dev_async(0, 0, t, 640)
    assert nu.update_wait() == 0


def test_without_a_reservation(hip):
    L = hip.lib()
    rig = Rig(hip, 4, SCHED["S"], 77, 4, reserve=False)
    nu = rig.nu
    taps = _noise(5700, nu.taps, rig.dt)
    p = taps.ctypes.data_as(C.c_void_p)
    assert nu.update_buffer() is None
    assert L.bfhip_nupc_update_coeff_async(nu.h, 0, 2, p, nu.taps) == ESTATE
    assert L.bfhip_nupc_update_coeff_dev_async(nu.h, 0, 2, p, nu.taps, None) == ESTATE
    assert b"reserve_update" in L.bfhip_nupc_last_error()
    assert L.bfhip_nupc_update_wait(nu.h) == ESTATE and L.bfhip_nupc_update_result(nu.h) == ESTATE
    assert not nu.update_busy()
    nu.update_coeff(0, 2, taps)                                # the synchronous call is as before


@pytest.mark.parametrize("key", ["S", "B"])
def test_a_non_finite_rewrite_cannot_go_live(hip, key):
    L = hip.lib()
    n_blocks = PLAN[key][0]
    rig = Rig(hip, 4, SCHED[key], 87, n_blocks)
    nu = rig.nu
    bad = _noise(5800, nu.taps, rig.dt)
    bad[nu.taps - 5] = np.nan                                  # in the last segment's last partition
    good = _noise(5801, nu.taps, rig.dt)

    def poison(r):
        nu.update_coeff_async(1, 2, bad)
        assert L.bfhip_nupc_update_wait(nu.h) == EINVAL
        assert NAN_MSG in L.bfhip_nupc_last_error()
        assert L.bfhip_nupc_update_result(nu.h) == EINVAL and NAN_MSG in L.bfhip_nupc_last_error()
        assert L.bfhip_nupc_set_coeff(nu.h, 1, 2) == ESTATE
        nu.set_coeff(0, 2)                                     # other sets are not affected
        r.req[0] = 2

    def heal(r):
        assert L.bfhip_nupc_set_coeff(nu.h, 1, 2) == ESTATE    # still refused
        nu.update_coeff_async(1, 2, good)
        r.h[1][2] = good
        assert nu.update_wait() == 0
        r.request({1: 2})

    raw = rig.run({1: poison, PLAN[key][2] + (4 if key == "B" else 0): heal})
    assert len(rig.switches) == 2
    got = _frames(raw, rig.dt)
    assert np.all(np.isfinite(got))
    _check(got, rig.want(), 4, rig.L0)


def test_every_allocation_failure_of_the_reservation_is_an_error_code(hip):
    """bfhip_selftest_fail_alloc on the allocations finalize makes for the reservation (they come
    last in finalize, so they are the ones past a life without it): finalize fails with a code,
    destroy frees, and a clean life rewrites and switches afterwards"""
    L = hip.lib()
    h = _noise(9, 57344, np.float32)

    def life(reserve, blocks=0):
        nu = None
        try:
            nu = hip.Nupc(*SCHED["B"], 4, 1, 1)
            if reserve:
                nu.reserve_update()
            nu.add_filter(0, 0, h)
            nu.add_coeff(0, h[::-1])
            nu.finalize()
            out = []
            if blocks:
                nu.update_coeff_async(0, 1, h * 0.5)
                assert nu.update_wait() == 0
                nu.set_coeff(0, 1)
                x = np.full((4096, 1), 0.25, np.float32)
                out = [nu.block(x)[1] for _ in range(blocks)]
        finally:
            left = L.bfhip_selftest_fail_alloc(0)
            if nu is not None:
                nu.close()
        return left, out

    big = 1000000
    made = []
    for reserve in (False, True):
        L.bfhip_selftest_fail_alloc(big)
        made.append(big - life(reserve)[0])
    print("allocations up to the end of finalize: %d without the reservation, %d with" % tuple(made))
    assert made[1] >= made[0] + 3                  # the two staging buffers and the result words at least
    for n in range(made[0] + 1, made[1] + 1):
        L.bfhip_selftest_fail_alloc(n)
        with pytest.raises(hip.BfhipError):
            life(True)
    _, out = life(True, blocks=3)
    assert len(out) == 3 and np.all(np.isfinite(np.frombuffer(np.concatenate(out).tobytes(), np.float32)))
