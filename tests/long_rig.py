"""The rig the long-window test files share (test_gpu_long_window_ref.py, test_gpu_lookahead_ref.py):
one crossbar configuration built as an engine on any long-window plan and as the float64 model
(tests/xbar_ref.py), driven with the same blocks and control calls.

Plans: "std" (BFHIP_LONG_WINDOW=0), "long" (4-block windows, no look-ahead), "la" (single-tier
look-ahead MAC), "far" (look-ahead with the far tier).  Named as a string, a plan sets
BFHIP_LONG_WINDOW, BFHIP_LOOKAHEAD, BFHIP_LOOKAHEAD_FAR and BFHIP_MAC_TARGET_WGS (one chunk per group:
the long plan takes whole entries only, and the standard engine next to it is held to the same cut).
True / False stand for "long" / "std" with the look-ahead knobs left at "by volume" and the MAC's
workgroup target untouched: what test_gpu_long_window_ref.py has always run."""
import collections

import numpy as np

import brutefir_amd as bf
import cases
import xbar_ref as xr

L = 8192
TOL_BLOCK, TOL_RUN = 2e-5, 1e-5
PLANS = {"std": ("0", "0", "0"), "long": ("1", "0", "0"), "la": ("1", "1", "0"), "far": ("1", "1", "1")}


def _ir(seed, taps, n_in):
    return cases.make_ir(np.random.default_rng(seed), taps, n_in)


def flat_ir(seed, taps, n_in):
    """white noise of unit energy over n_in inputs: every partition carries the same weight"""
    return np.random.default_rng(seed).standard_normal(taps) / np.sqrt(taps) / n_in


IRS = {"decay": _ir, "flat": flat_ir}

# what drive() records: outputs [frames][O] in the output format's units, and per block the status,
# window_blocks, lookahead_blocks, lookahead_far_blocks and mac_counts (launches, head blocks, full blocks)
Run = collections.namedtuple("Run", "y sts wins la far counts")


class Rig:
    """one crossbar configuration: sets (o, i) and extra sets ("x", k), filter f = o * I + i"""

    def __init__(self, N, I, O, seed=1000, delays=None, lengths=None, gain=1.0, n_extra=0, crossfade=False,
                 infmt="S24_4LE", outfmt="FLOAT_LE", ir="decay"):
        self.N, self.I, self.O = N, I, O
        self.infmt, self.outfmt, self.crossfade = infmt, outfmt, crossfade      # crossfade: all, none, or a set of filters
        self.delays = delays or {}
        self.ir = IRS[ir]
        self.sets = {}
        for o in range(O):
            for i in range(I):
                n = (lengths or {}).get((o, i), L * N)
                self.sets[(o, i)] = self.ir(seed + o * I + i, n, I) * gain
        for k in range(n_extra):
            self.sets[("x", k)] = self.ir(seed + 7919 + k, L * N, I) * gain
        self.model = [xr.Filter(i, o, self.sets[(o, i)], self.delay(o, i)) for o in range(O) for i in range(I)]
        self.uses = [(o, i) for o in range(O) for i in range(I)]

    def delay(self, o, i):
        d = self.delays
        return d.get((o, i), d.get(i, 0)) if isinstance(d, dict) else 0

    def fades(self, f):
        return self.crossfade if isinstance(self.crossfade, bool) else f in self.crossfade

    def engine(self, monkeypatch, plan, env=None, setup=None, sets_hook=None):
        """plan: "std", "long", "la", "far" (or True / False: see the module docstring)"""
        if isinstance(plan, str):
            lw, la, far = PLANS[plan]
            monkeypatch.setenv("BFHIP_LONG_WINDOW", lw)
            monkeypatch.setenv("BFHIP_LOOKAHEAD", la)
            monkeypatch.setenv("BFHIP_LOOKAHEAD_FAR", far)
            monkeypatch.setenv("BFHIP_MAC_TARGET_WGS", str(16 * ((self.O + 7) // 8) * self.I))
        else:
            monkeypatch.setenv("BFHIP_LONG_WINDOW", "1" if plan else "0")
            for k in ("BFHIP_LOOKAHEAD", "BFHIP_LOOKAHEAD_FAR"):
                monkeypatch.delenv(k, raising=False)
        for k in ("BFHIP_OVERLAP", "BFHIP_DEFER", "BFHIP_LONG_CHUNKS", "BFHIP_TEST_WRAP_PERIODS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        e = bf.Engine(L, self.N, 4, self.I, self.O)
        if setup:
            setup(e)
        else:
            e.set_interleaved(0, self.infmt)
        e.set_interleaved(1, self.outfmt)
        e.cid = {}
        for key, h in self.sets.items():
            e.cid[key] = e.add_coeff(h)
        if sets_hook:
            sets_hook(e)
        for o in range(self.O):
            for i in range(self.I):
                e.add_filter(in_ch=[i], out_ch=[o], coeff=e.cid[(o, i)], delayblocks=self.delay(o, i),
                             crossfade=self.fades(o * self.I + i))
        e.finalize()
        return e

    # ---- control calls, applied to an engine and (once) to the model
    def act(self, e, a):
        if a[0] == "coeff":
            e.set_coeff(a[1], e.cid[a[2]])
        elif a[0] == "rewrite":
            e.update_coeff_block(e.cid[a[1]], a[2], a[3])
        elif a[0] == "delay":
            e.set_delayblocks(a[1], a[2])
        elif a[0] == "scale":
            e.set_scale(a[1], a[2], a[3], a[4])
        else:
            raise ValueError(a)

    def model_act(self, t, a):
        if a[0] == "coeff":
            self.uses[a[1]] = a[2]
            self.model[a[1]].change(t, fade=self.fades(a[1]), taps=self.sets[a[2]])
        elif a[0] == "rewrite":
            h = self.sets[a[1]].copy()
            h[a[2] * L:(a[2] + 1) * L] = a[3]
            self.sets[a[1]] = h
            for f, key in enumerate(self.uses):
                if key == a[1]:
                    self.model[f].change(t, taps=h)
        elif a[0] == "delay":
            self.model[a[1]].change(t, delay=a[2])
        elif a[0] == "scale":
            self.model[a[1]].set_scale(t, a[2], a[3], a[4])
        else:
            raise ValueError(a)

    def expect(self, blocks, actions=None, x=None):
        for t in sorted(actions or {}):
            for a in actions[t]:
                self.model_act(t, a)
        if x is None:
            x = xr.decode(np.concatenate(blocks), self.infmt, self.I)
        return xr.output(x, self.model, L, self.N, self.O, len(blocks))


def drive(rig, e, blocks, actions=None, rt=None, before=None):
    """-> Run.  rt: real-time flags for the whole run, or [(first block, one past the last, flags)]
    intervals with plain block() calls around them.  before: {block: callable(engine)} run ahead of the
    block's control calls (what the model does not see: prewarm)"""
    outs, sts, wins, la, far, counts = [], [], [], [], [], []
    spans = [(0, len(blocks), rt)] if rt is not None and not isinstance(rt, (list, tuple)) else list(rt or ())
    on = None                                    # flags of the interval in force
    pending = 0

    def take(r):
        sts.append(r[0])
        outs.append(r[1])

    def leave():
        nonlocal pending, on
        while pending:
            take(e.rt_wait())
            pending -= 1
        e.rt_end()
        on = None

    for k, b in enumerate(blocks):
        want = next((f for a, z, f in spans if a <= k < z), None)
        if on is not None and want != on:
            leave()
        if want is not None and on is None:
            e.rt_begin(want)
            on = want
        if before and k in before:
            before[k](e)
        for a in (actions or {}).get(k, ()):
            rig.act(e, a)
        if on is not None and on & bf.RT_OVERLAP:
            e.rt_submit(b)
            pending += 1
            if pending == 2:
                take(e.rt_wait())
                pending -= 1
        elif on is not None:
            take(e.rt_block(b))
        else:
            take(e.block(b))
        wins.append(e.window_blocks)
        la.append(e.lookahead_blocks)
        far.append(e.lookahead_far_blocks)
        counts.append(e.mac_counts)
    if on is not None:
        leave()
    e.sync()
    y = xr.decode(np.concatenate(outs), rig.outfmt, rig.O)
    return Run(y, sts, wins, la, far, counts)


def errors(got, want):
    """-> (worst relative RMS error of a block, relative RMS error over the run)"""
    worst = max(cases.rel_rms(got[k * L:(k + 1) * L], want[k * L:(k + 1) * L]) for k in range(len(want) // L))
    return worst, cases.rel_rms(got, want)


def hold(got, want, label="", tol_block=TOL_BLOCK, tol_run=TOL_RUN):
    assert cases.rel_rms(got, want) <= tol_run, label
    for k in range(len(want) // L):
        s = slice(k * L, (k + 1) * L)
        err = cases.rel_rms(got[s], want[s])
        assert err <= tol_block, (label, k, err)


def both(monkeypatch, rig, blocks, actions=None, env=None, win=None, rt=None):
    """run the long and the standard engine, hold both to the model; win(k) -> the plan expected at
    block k on the long engine (4 or 2), default 4 everywhere"""
    got = {}
    for long in (True, False):
        e = rig.engine(monkeypatch, long, env)
        r = drive(rig, e, blocks, actions, rt)
        assert r.sts == [0] * len(blocks), (long, r.sts)
        if long:
            want_w = [win(k) if win else 4 for k in range(len(blocks))]
            assert r.wins == want_w, r.wins
        else:
            assert set(r.wins) == {2}
        got[long] = (r.y, e)
    want = rig.expect(blocks, actions)
    for long in (True, False):
        hold(got[long][0], want, "long" if long else "standard")
    for long in (True, False):
        got[long][1].close()
    return got[True][0], got[False][0], want


def blocks_for(rig, n, seed=7, amplitude=0.1):
    return cases.raw_blocks(seed, n, L, rig.I, rig.infmt, amplitude=amplitude)
