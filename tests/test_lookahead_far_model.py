"""float64 model of the two-tier look-ahead schedule of the long-window MAC (kernels.h: mac_la_kernel with
its third phase bit, la_far_phase; passes.hip: do_mac, la_prime and the two validity tables), against direct
convolution.

Call t runs, for the entries of near slice t mod 3, partition 1 of blocks t+1 .. t+3 into
near[(t+k) mod 4][t mod 3], and for the entries of far slice t mod 6 the partitions p >= 2 of blocks
t+1 .. t+6 into far[(t+k) mod 7][t mod 6].  The block's own output is the head pass -- ((near0 + near1) +
near2) + far0 + .. + far5 + partition 0 of every entry -- when all nine buffers were computed for block t
at the current epoch, else the full long MAC.  Everything that changes a product already stored bumps the
epoch.  The model counts every buffer write and checks every read."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_lookahead_model import B, Model, expected, slices  # noqa: E402


def far_slices(n):
    b, r = divmod(n, 6)
    out, first = [], 0
    for j in range(6):
        m = b + (1 if j < r else 0)
        out.append(range(first, first + m))
        first += m
    return out


def far_gate(N, delays=(0,)):
    """the engine's gate: some entry has three long partitions or more, and every p >= 2 of every entry
    reaches back six blocks or more (only the last one is shifted: 3p - shift + delay >= 6)"""
    any3 = False
    for d in delays:
        P = N - d                                    # standard partitions the entry uses
        maxP, shift = (P + 2) // 3, 3 * ((P + 2) // 3) - P
        any3 = any3 or maxP >= 3
        if maxP >= 3 and 3 * (maxP - 1) - shift + d < 6:
            return False
    return any3


class FarModel(Model):
    def __init__(self, x, h, delays, N, prime=False):
        super().__init__(x, h, delays, N)
        self.F = {}                      # (slot, slice) -> [value, block, epoch]
        self.far_writes = {}
        self.primed = set()              # buffers the start zeroed (the pass that follows may store them again)
        if prime:
            # no block exists: the tails of the first three (near) and six (far) blocks read silence alone
            for t in range(3):
                for j in range(3):
                    self.A[t % 4, j] = [np.zeros(2 * B + 1, complex), t, self.epoch]
                    self.primed.add(("near", t, j))
            for t in range(6):
                for j in range(6):
                    self.F[t % 7, j] = [np.zeros(2 * B + 1, complex), t, self.epoch]
                    self.primed.add(("far", t, j))

    def call(self, t, standard=False):
        if standard:
            return super().call(t, standard=True)
        self.feed(t)
        near = [self.A.get((t % 4, j)) for j in range(3)]
        far = [self.F.get((t % 7, j)) for j in range(6)]
        if all(b is not None and b[1] == t and b[2] == self.epoch for b in near + far):
            for j in range(3):                                     # written exactly once before it is read
                n = self.writes.get((t, j, self.epoch), 0)
                assert n == 1 or (n == 0 and ("near", t, j) in self.primed)
            for j in range(6):
                n = self.far_writes.get((t, j, self.epoch), 0)
                assert n == 1 or (n == 0 and ("far", t, j) in self.primed)
            Y = (near[0][0] + near[1][0]) + near[2][0]
            for j in range(6):
                Y = Y + far[j][0]
            for i in range(self.I):
                Y = Y + self.term(i, 0, t)
            self.heads += 1
        else:
            Y = np.zeros(2 * B + 1, complex)
            for i in range(self.I):
                for p in range(len(self.G[i])):
                    Y = Y + self.term(i, p, t)
            self.fulls += 1
        j = t % 3
        for k in (1, 2, 3):
            Z = np.zeros(2 * B + 1, complex)
            for i in slices(self.I)[j]:
                if len(self.G[i]) > 1:
                    q0, _ = self.G[i][1]
                    assert t + k - q0 - self.d[i] <= t            # the ring holds it already
                    Z = Z + self.term(i, 1, t + k)
            self.A[(t + k) % 4, j] = [Z, t + k, self.epoch]
            key = (t + k, j, self.epoch)
            self.writes[key] = self.writes.get(key, 0) + 1
        j = t % 6
        written = set()
        for k in range(1, 7):
            Z = np.zeros(2 * B + 1, complex)
            for i in far_slices(self.I)[j]:
                for p in range(2, len(self.G[i])):
                    q0, _ = self.G[i][p]
                    assert t + k - q0 - self.d[i] <= t
                    Z = Z + self.term(i, p, t + k)
            assert (t + k) % 7 != t % 7                           # never a buffer the head pass of this call read
            written.add((t + k) % 7)
            self.F[(t + k) % 7, j] = [Z, t + k, self.epoch]
            key = (t + k, j, self.epoch)
            self.far_writes[key] = self.far_writes.get(key, 0) + 1
        assert len(written) == 6
        return np.fft.irfft(Y)[:B] * (4 * B)


def run(N, I, event, phase, prime, T=None):
    rng = np.random.default_rng(N * 100 + I * 10 + phase)
    T = N + 18 if T is None else T
    x = rng.standard_normal((I, T, B))
    h = [rng.standard_normal(N * B) for _ in range(I)]
    delays = [int(v) for v in rng.integers(0, 3, I)]
    assert far_gate(N, delays)
    m = FarModel(x, h, delays, N, prime=prime)
    at = N + 1 + phase                   # six consecutive calls: once on each value of t mod 6
    got, states = [], []
    for t in range(T):
        if t == at and event in ("swap", "rewrite", "scale"):
            m.change(event, rng)
        got.append(m.call(t, standard=(event == "standard" and t == at)))
        states.append(([v.copy() for v in m.h], list(m.scale), list(m.d)))
    return m, np.array(got), expected(x, states, T), T


@pytest.mark.parametrize("N", [9, 11, 13, 20])
@pytest.mark.parametrize("I", [3, 8])
@pytest.mark.parametrize("event,phase", [(None, 0)] + [(ev, ph) for ev in ("swap", "rewrite", "scale", "standard")
                                                       for ph in range(6)])
def test_two_tier_schedule_is_the_linear_convolution(N, I, event, phase):
    prime = phase % 2 == 0
    m, got, want, T = run(N, I, event, phase, prime)
    assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    assert all(c == 1 for c in m.writes.values()) and all(c == 1 for c in m.far_writes.values())
    # an unprimed start costs six full blocks, an event six more (1.17 x a block each: the full MAC plus
    # one third of p = 1 and one sixth of p >= 2), a standard block six behind itself
    start = 0 if prime else 6
    if event is None:
        assert (m.fulls, m.heads) == (start, T - start)
    elif event == "standard":
        assert m.standards == 1 and m.fulls == start + 6 and m.heads == T - start - 7
    else:
        assert m.fulls == start + 6 and m.heads == T - start - 6


def test_sixths_are_contiguous_and_even():
    assert [len(s) for s in far_slices(64)] == [11, 11, 11, 11, 10, 10]
    assert [len(s) for s in far_slices(8)] == [2, 2, 1, 1, 1, 1]
    assert [len(s) for s in far_slices(3)] == [1, 1, 1, 0, 0, 0]
    for n in range(1, 70):
        assert [i for s in far_slices(n) for i in s] == list(range(n))
        assert max(len(s) for s in far_slices(n)) - min(len(s) for s in far_slices(n)) <= 1


def test_gate_arithmetic():
    assert not far_gate(8)                       # p = 2 is the last partition, shifted by one: reaches back 5
    assert all(far_gate(N) for N in (9, 11, 13, 20))
    assert not far_gate(8, [1])                  # 7 partitions behind a block of delay: p = 2 shifted by two reaches back 5
    assert far_gate(9, [1])                      # 8 partitions: p = 2 shifted by one, behind a block of delay, reaches back 6
    assert far_gate(9, [0, 2]) and not far_gate(8, [2, 0])     # one entry that fails is enough
    assert not far_gate(6) and not far_gate(4)   # two long partitions: nothing for the far tier
    assert far_gate(11, [0, 1, 2])


def test_stale_far_buffers_are_never_read():
    """after an epoch bump no head pass runs until six far passes have refilled the block's buffers"""
    rng = np.random.default_rng(1)
    N, I, T = 11, 8, 30
    m = FarModel(rng.standard_normal((I, T, B)), [rng.standard_normal(N * B) for _ in range(I)], [0] * I, N)
    kinds = []
    for t in range(T):
        if t == 13:
            m.change("swap", rng)
        before = m.heads
        m.call(t)
        kinds.append(m.heads > before)
    assert kinds == [False] * 6 + [True] * 7 + [False] * 6 + [True] * (T - 19)
