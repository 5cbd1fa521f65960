"""CPU: the non-uniform convolver's period schedule (csrc/nupc_sched.h) -- the switch scheduler, the
gain-ramp mirror and the delay machine -- compiled by g++ alone into tests/chost/nupc_sched_driver.cpp, once
plainly and once with -fsanitize=address,undefined, and run as a program of its own.  Nothing is loaded into
Python.  What the schedule should decide is worked out here: switch frames from nupc_stagger_ref, per-block
modes and the end of a switch from frame ranges, delayed blocks from the oracle's bfo_delay."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bforacle as bo
import nupc_stagger_ref as sr
from nupc_stagger_ref import SMALL, ZERO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "brutefir_amd", "csrc", "nupc_sched.h")
DRIVER = os.path.join(ROOT, "tests", "chost", "nupc_sched_driver.cpp")
SCHEDULES = [SMALL, ZERO, ([64, 128, 256, 512, 1024], [2, 2, 2, 2, 3]), ([64, 256], [5, 2])]
ALIGNED, STAGGERED = 0, 1
L0 = 64


def _compile(out, flags, link=True):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags + \
          ["-I" + os.path.dirname(HEADER), DRIVER] + (["-o", out] if link else ["-c", "-o", out])
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nupc_sched") / request.param)
    b = _compile(exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else [])
    assert b.returncode == 0, b.stderr[-3000:]

    def run(cmd, numbers):
        r = subprocess.run([exe, cmd], input=" ".join(str(v) for v in numbers) + "\n", capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "nupc_sched_driver: clean"
        return lines[:-1]
    return run


def _sched(s):
    return [len(s[0])] + list(s[0]) + list(s[1])


# ---------------------------------------------------------------- no HIP in the header

def test_the_header_includes_no_hip_header_and_has_no_device_code():
    text = open(HEADER).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r'#include\s*[<"][^>"]*hip/', code)
    assert "__device__" not in code and "__global__" not in code
    assert "hip_runtime" not in code


def test_the_drivers_object_references_no_hip_symbol(tmp_path):
    obj = str(tmp_path / "nupc_sched_driver.o")
    b = _compile(obj, [], link=False)
    assert b.returncode == 0, b.stderr[-3000:]
    syms = subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout
    assert syms and "hip" not in syms.lower(), [s for s in syms.splitlines() if "hip" in s.lower()]


# ---------------------------------------------------------------- switch frames

@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda s: "x".join(map(str, s[0])))
def test_switch_frames(driver, sched):
    treqs = [b * L0 for b in range(70)]
    for mode in (STAGGERED, ALIGNED):
        lines = driver("frames", _sched(sched) + [mode, len(treqs)] + treqs)
        assert len(lines) == len(treqs)
        for t_req, ln in zip(treqs, lines):
            got = [int(v) for v in ln.split()]
            want = sr.switch_frames(sched, t_req)
            assert want == sr.switch_frames_walk(sched, t_req)
            if mode == STAGGERED:
                assert got == [t_req] + want, t_req
            else:
                t_sw = max(max(want), t_req)
                assert got == [t_sw] * (1 + len(want)), t_req


# ---------------------------------------------------------------- per-block modes, the end of a switch, the ring flip

def _blocks(sched, first_period, last_period):
    """(period, segment, pos, L) of every segment block launched in the periods [first, last)"""
    out = []
    for p in range(first_period, last_period):
        end = (p + 1) * L0
        for k, (L, off) in enumerate(zip(sched[0], sr.offsets(sched))):
            if end % L == 0:
                out.append((p, k, end - L + off, L))
    return out


def _meets(pos, L, a, b):
    """does the frame range [pos, pos + L) meet [a, b)?"""
    return max(pos, a) < min(pos + L, b)


@pytest.mark.parametrize("mode", [ALIGNED, STAGGERED], ids=["aligned", "staggered"])
@pytest.mark.parametrize("fade", [0, 2, 64, 323])
@pytest.mark.parametrize("commit", [5, 7, 16])
@pytest.mark.parametrize("sched", SCHEDULES, ids=lambda s: "x".join(map(str, s[0])))
def test_block_modes_and_the_end_of_a_switch(driver, sched, commit, fade, mode):
    periods = commit + 80
    lines = driver("walk", _sched(sched) + [mode, fade, commit, periods])
    B = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln[0] == "B"]
    E = {int(ln.split()[1]): tuple(int(v) for v in ln.split()[2:]) for ln in lines if ln[0] == "E"}
    P = {int(ln.split()[1]): tuple(int(v) for v in ln.split()[2:]) for ln in lines if ln[0] == "P"}
    t_req = commit * L0
    t_seg = sr.switch_frames(sched, t_req)
    t_sw = max(max(t_seg), t_req)
    if mode == ALIGNED:
        t_seg = [t_sw] * len(t_seg)
    want_blocks = _blocks(sched, 0, periods)
    assert [(p, k, pos) for p, k, pos, *_ in B] == [(p, k, pos) for p, k, pos, _ in want_blocks]

    # the old assignment is needed by a block iff the block has frames below its segment's t + F; the last
    # frame the old assignment writes (aligned: the old ring has to be emitted down to there)
    def needs_old(k, pos):
        return pos < t_seg[k] + fade
    later = _blocks(sched, periods, periods + 300)
    old_hi = t_sw
    busy_want = {}
    for p in range(periods):
        if p < commit:
            busy_want[p] = False
            continue
        for q, k, pos, L in want_blocks:
            if q == p and mode == ALIGNED and needs_old(k, pos):
                old_hi = max(old_hi, pos + L)
        end = (p + 1) * L0
        old_left = any(needs_old(k, pos) for q, k, pos, L in want_blocks + later if q > p)
        if mode == ALIGNED:
            busy_want[p] = old_left or end < max(t_sw + fade, old_hi)
        else:
            busy_want[p] = fade > 0 and old_left
    flips = 0
    for p in range(periods):
        busy, cur = P[p]
        assert bool(busy) == busy_want[p], p
        flips += cur != (P[p - 1][1] if p else 0)
        in_switch = p >= commit and (p == commit or busy_want[p - 1]) and (mode == ALIGNED or fade > 0)
        two_rings, rel0 = E[p]
        assert bool(two_rings) == (in_switch and mode == ALIGNED), p
        assert rel0 == (p * L0 - t_sw if two_rings else 0), p
    assert flips == (1 if mode == ALIGNED else 0)
    assert not P[periods - 1][0]                                  # every switch here ends within 80 periods
    # sw falls in the FIRST such period: the period before still had something left
    ends = [p for p in range(commit, periods) if not busy_want[p]]
    assert ends and (ends[0] == commit or busy_want[ends[0] - 1])

    seen = set()
    for (p, k, pos, got_mode, ring, ring2, is_fade, t_k), (_, _, _, L) in zip(B, want_blocks):
        in_switch = p >= commit and (p == commit or busy_want[p - 1]) and (mode == ALIGNED or fade > 0)
        cur = P[p - 1][1] if p else 0                              # the live ring when the block is planned
        if not in_switch:
            want = 1
        elif _meets(pos, L, t_seg[k], t_seg[k] + fade):
            want = 2
        elif mode == ALIGNED and pos < t_sw + fade and pos + L <= t_sw:
            want = 0
        else:
            want = 1
        assert got_mode == want, (p, k, pos)
        seen.add(want if in_switch else None)
        assert is_fade == (want == 2 and mode == STAGGERED)
        if p >= commit:
            assert t_k == t_seg[k]
        if mode == STAGGERED or not in_switch:
            assert (ring, ring2) == (cur, -1)                      # everything goes into the live ring
        else:
            assert (ring, ring2) == {0: (cur, -1), 1: (1 - cur, -1), 2: (cur, 1 - cur)}[want]
    if fade > 0:
        assert 2 in seen
    if mode == ALIGNED and t_sw > t_req:
        assert 0 in seen                                           # the first segment's block at t_req, at least


# ---------------------------------------------------------------- the delay machine against the oracle's bfo_delay

def _oracle_delay(F, ss, init, maxd, reqs, mutes, mute_first, data):
    lib = bo.lib()
    lib.bfo_delay_new.restype = C.c_void_p
    lib.bfo_delay_new.argtypes = [C.c_int] * 4
    lib.bfo_delay_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.bfo_delay_free.argtypes = [C.c_void_p]
    d = lib.bfo_delay_new(F, init, maxd, ss)
    out = []
    for blk, req, muted in zip(data, reqs, mutes):
        b = blk.copy()
        if muted and mute_first:
            b[:] = 0                                               # input side: zeros enter the line
        lib.bfo_delay_update(d, b.ctypes.data, int(req))
        if muted and not mute_first:
            b[:] = 0                                               # output side: the delayed block is muted
        out.append(b)
    lib.bfo_delay_free(d)
    return out


@pytest.mark.parametrize("mute_first", [1, 0], ids=["input_side", "output_side"])
@pytest.mark.parametrize("maxd", [-1, 0, 40, 64, 200])
@pytest.mark.parametrize("ss", [2, 3, 4, 8])
def test_delay_machine_is_the_oracles(driver, ss, maxd, mute_first):
    F, periods = 64, 60
    rng = np.random.default_rng(1000 * ss + 10 * (maxd + 1) + mute_first)
    # (an initial delay above a maxdelay > 0 is refused by the configuration parser: delay.c has no answer to it)
    init = int(rng.integers(0, (maxd if maxd > 0 else 150) + 1))
    top = max(maxd, 0) + 30                                        # requests above maxdelay are part of the walk
    reqs, req = [], init
    for p in range(periods):
        if rng.random() < 0.3:
            req = int(rng.choice([int(rng.integers(0, top + 1)), 0, F - 1, F, F + 1, max(maxd, 0), max(maxd, 0) + 1]))
        reqs.append(req)
    mutes = [1 if 20 <= p < 27 or p == 41 else 0 for p in range(periods)]
    data = rng.integers(1, 255, (periods, F * ss), dtype=np.uint8)
    numbers = [F, ss, maxd, init, mute_first, periods]
    for p in range(periods):
        numbers += [reqs[p], mutes[p], data[p].tobytes().hex()]
    lines = driver("delay", numbers)
    want = _oracle_delay(F, ss, init, maxd, reqs, mutes, mute_first, data)
    assert len(lines) == periods
    for p, ln in enumerate(lines):
        assert ln.split()[0] == want[p].tobytes().hex(), (p, reqs[p], ln.split()[1])
    if maxd > 0:
        assert len({ln.split()[1] for ln in lines}) >= 3           # the delay in force did change


# ---------------------------------------------------------------- the gain mirror

def test_gain_mirror_follows_the_device_records(driver):
    n_ch, periods = 3, 60
    rng = np.random.default_rng(5)
    events = [(0, 1, 0, 200)]                                      # (period, kind, channel, value)
    for p in range(2, periods, 3):
        events.append((p, 0, int(rng.integers(0, n_ch)), int(rng.integers(-2000, 2001))))
        if p % 4 == 0:
            events.append((p, 1, 0, int(rng.choice([0, 1, 2, 63, 64, 65, 200, 1000]))))
    events += [(31, 0, 1, 700), (32, 0, 1, -300)]                  # a second request in mid-ramp
    lines = driver("gain", [n_ch, L0, periods, len(events)] + [v for e in events for v in e])
    G = [tuple(int(v) for v in ln.split()[1:]) for ln in lines]
    assert len(G) == n_ch * periods
    # done is min(len, frames emitted since the ramp began): it only grows by L0 or saturates within a ramp
    ramps = 0
    prev = {ch: (0, 0) for ch in range(n_ch)}
    for p, ch, done, ln in G:
        pd, pl = prev[ch]
        assert done == min(ln, pd + L0) or done == min(ln, L0), (p, ch)
        ramps += ln > L0 and done == L0
        prev[ch] = (done, ln)
    assert ramps >= 3
