"""float64 model of the look-ahead schedule of the long-window MAC (kernels.h: mac_la_head_kernel,
mac_la_tail_kernel; passes.hip: do_mac and its validity table), against direct convolution.

Call t runs, for the entries of slice t mod 3, the tail partitions (p >= 1) of blocks t+1, t+2, t+3 and
stores them in the ahead buffers A[(t+k) mod 4][t mod 3]; the block's own output is the head pass
(partition 0 of every entry on top of A[t mod 4][0..2]) when all three buffers were computed for block t
at the current epoch, else the full long MAC.  Everything that changes a product already stored bumps
the epoch.  The model counts every buffer write and checks every read."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_long_window_model import direct, from_std, std_spectra  # noqa: E402

B = 8


def slices(n):
    b, r = divmod(n, 3)
    out, first = [], 0
    for j in range(3):
        m = b + (1 if j < r else 0)
        out.append(range(first, first + m))
        first += m
    return out


class Model:
    """one output fed by I inputs (entry i: input i, delay d[i], taps h[i], scale s[i])"""

    def __init__(self, x, h, delays, N):
        self.x, self.N, self.I = x, N, len(h)
        self.h = [v.copy() for v in h]
        self.scale = [1.0] * self.I
        self.d = list(delays)
        self.W = {}                      # (input, block) -> long window spectrum
        self.X = {}                      # (input, block) -> standard window spectrum
        self.A = {}                      # (slot, slice) -> [value, block, epoch]
        self.epoch = 1
        self.writes = {}                 # (block, slice, epoch) -> count
        self.heads = self.fulls = self.standards = 0
        self.derive()

    def derive(self):
        self.H = [std_spectra(self.h[i], B, self.N) for i in range(self.I)]
        self.G = [from_std(self.H[i], B, self.N - self.d[i]) for i in range(self.I)]

    def change(self, what, rng):
        if what == "swap":
            self.h[1] = rng.standard_normal(self.N * B)
        elif what == "rewrite":
            self.h[0][4 * B:5 * B] = rng.standard_normal(B)
        elif what == "scale":
            self.scale[self.I - 1] = 0.5
        self.derive()
        self.epoch += 1

    def blk(self, i, t):
        return self.x[i][t] if t >= 0 else np.zeros(B)

    def feed(self, t):
        for i in range(self.I):
            self.W[i, t] = np.fft.rfft(np.concatenate([self.blk(i, t - k) for k in (3, 2, 1, 0)]))
            self.X[i, t] = np.fft.rfft(np.concatenate([self.blk(i, t - 1), self.blk(i, t)]))

    def term(self, i, p, t):
        q0, Gp = self.G[i][p]
        s = t - q0 - self.d[i]
        return self.scale[i] * self.W[i, s] * Gp if (i, s) in self.W else 0.0

    def call(self, t, standard=False):
        self.feed(t)
        if standard:
            # the standard MAC: 2B windows, standard partitions; nothing is computed ahead
            self.epoch += 1
            self.standards += 1
            Y = np.zeros(B + 1, complex)
            for i in range(self.I):
                for q in range(self.N - self.d[i]):
                    if (i, t - q - self.d[i]) in self.X:
                        Y += self.scale[i] * self.X[i, t - q - self.d[i]] * self.H[i][q]
            return np.fft.irfft(Y)[:B] * (2 * B)
        bufs = [self.A.get((t % 4, j)) for j in range(3)]
        if all(b is not None and b[1] == t and b[2] == self.epoch for b in bufs):
            for j in range(3):
                assert self.writes[t, j, self.epoch] == 1          # written exactly once before it is read
            Y = (bufs[0][0] + bufs[1][0]) + bufs[2][0]
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
                for p in range(1, len(self.G[i])):
                    q0, _ = self.G[i][p]
                    assert t + k - q0 - self.d[i] <= t            # the ring holds it already
                    Z = Z + self.term(i, p, t + k)
            self.A[(t + k) % 4, j] = [Z, t + k, self.epoch]
            key = (t + k, j, self.epoch)
            self.writes[key] = self.writes.get(key, 0) + 1
        return np.fft.irfft(Y)[:B] * (4 * B)


def expected(x, states, T):
    """states[t] = (taps, scales, delays) in force at block t: the filter over the whole input history"""
    out = np.zeros((T, B))
    for t in range(T):
        h, sc, d = states[t]
        for i in range(len(h)):
            out[t] += sc[i] * direct(list(x[i][:t + 1]), h[i][:(len(h[i]) // B - d[i]) * B], B, d[i])[t]
    return out


@pytest.mark.parametrize("N", [8, 11, 13, 32])
@pytest.mark.parametrize("I", [2, 8])
@pytest.mark.parametrize("event,phase", [(None, 0)] + [(ev, ph) for ev in ("swap", "rewrite", "scale", "standard")
                                                       for ph in (0, 1, 2)])
def test_lookahead_schedule_is_the_linear_convolution(N, I, event, phase):
    rng = np.random.default_rng(N * 100 + I * 10 + phase)
    T = N + 12
    x = rng.standard_normal((I, T, B))
    h = [rng.standard_normal(N * B) for _ in range(I)]
    delays = [int(v) for v in rng.integers(0, 3, I)]
    m = Model(x, h, delays, N)
    at = N + 1 + phase                   # three consecutive calls: once on each value of t mod 3
    got, states = [], []
    for t in range(T):
        if t == at and event in ("swap", "rewrite", "scale"):
            m.change(event, rng)
        got.append(m.call(t, standard=(event == "standard" and t == at)))
        states.append(([v.copy() for v in m.h], list(m.scale), list(m.d)))
    want = expected(x, states, T)
    assert np.abs(np.array(got) - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    # start: three full blocks, then heads; an event costs three more full blocks (1.33 x a block each:
    # the full MAC plus one third of the tails), a standard block two (itself, then slices to refill)
    assert all(c == 1 for c in m.writes.values())
    if event is None:
        assert (m.fulls, m.heads) == (3, T - 3)
    elif event == "standard":
        assert m.standards == 1 and m.fulls == 3 + 3 and m.heads == T - 7
    else:
        assert m.fulls == 3 + 3 and m.heads == T - 6


def test_slices_are_contiguous_and_even():
    assert [len(s) for s in slices(64)] == [22, 21, 21]
    assert [len(s) for s in slices(8)] == [3, 3, 2]
    assert [len(s) for s in slices(2)] == [1, 1, 0]
    for n in range(1, 70):
        assert [i for s in slices(n) for i in s] == list(range(n))


def test_stale_buffers_are_never_read():
    """after an epoch bump no head pass runs until three tail passes have refilled the block's buffers"""
    rng = np.random.default_rng(1)
    N, I, T = 8, 8, 20
    m = Model(rng.standard_normal((I, T, B)), [rng.standard_normal(N * B) for _ in range(I)], [0] * I, N)
    kinds = []
    for t in range(T):
        if t == 9:
            m.change("swap", rng)
        before = m.heads
        m.call(t)
        kinds.append(m.heads > before)
    assert kinds == [False] * 3 + [True] * 6 + [False] * 3 + [True] * (T - 12)
