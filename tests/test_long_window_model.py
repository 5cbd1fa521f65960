"""float64 model of the long-window overlap-save scheme the crossbar engine runs for large f32
crossbars (kernels.h: io_long_kernel, coeff_long_kernel, mac_xbar_kernel with ring step 3), against
direct convolution.

Window of an input at block t: w_t = [x_(t-3) | x_(t-2) | x_(t-1) | x_t] (4B reals).  Long partition p
holds the standard partitions 3p, 3p+1, 3p+2 (taps [3pB, 3pB + 3B)) placed as a standard partition
sits in its 2B window -- B zeros, then the taps -- over 4B; the last one is aligned to the end of the
filter (standard partitions q_end-3 .. q_end-1, those below 3p zero) and reads the window that many
blocks later, so that no window reaches further back than the standard scheme's N blocks.  The long
partitions are derived from the standard spectra (inverse 2B-point transform, re-window, forward
4B-point transform), which must agree with a derivation from the taps."""
import numpy as np
import pytest


def std_spectra(h, B, P):
    out = []
    for q in range(P):
        g = np.zeros(2 * B)
        g[B:] = h[q * B:(q + 1) * B]
        out.append(np.fft.rfft(g) / (2 * B))
    return out


def long_layout(q_end):
    """(first standard partition, first one that belongs to it) of every long partition"""
    PL = (q_end + 2) // 3
    return [((q_end - 3 if p == PL - 1 else 3 * p), 3 * p) for p in range(PL)]


def long_partitions(B, q_end, block_taps):
    """block_taps(q) -> the B taps of standard partition q"""
    G = []
    for q0, own in long_layout(q_end):
        g = np.zeros(4 * B)
        for jj in range(3):
            q = q0 + jj
            if own <= q < q_end:
                g[B + jj * B:B + (jj + 1) * B] = block_taps(q)
        G.append((q0, np.fft.rfft(g) / (4 * B)))
    return G


def from_std(H, B, q_end):
    return long_partitions(B, q_end, lambda q: np.fft.irfft(H[q] * (2 * B))[B:])


def from_taps(h, B, q_end):
    return long_partitions(B, q_end, lambda q: h[q * B:(q + 1) * B])


def run_long(x, B, G_of_block, delay):
    """x: [T][B]; G_of_block(t) -> long partitions in force at block t; output blocks [T][B]"""
    T = len(x)
    blk = lambda t: x[t] if t >= 0 else np.zeros(B)              # noqa: E731
    W = {t: np.fft.rfft(np.concatenate([blk(t - 3), blk(t - 2), blk(t - 1), blk(t)])) for t in range(-40, T)}
    out = []
    for t in range(T):
        Y = np.zeros(2 * B + 1, complex)
        for q0, Gp in G_of_block(t):
            s = t - q0 - delay
            if s >= 0:
                Y += W[s] * Gp
        out.append(np.fft.irfft(Y)[:B] * (4 * B))
    return np.array(out)


def direct(x, h, B, delay):
    y = np.convolve(np.concatenate(x), h)[:len(x) * B]
    y = np.concatenate([np.zeros(delay * B), y])[:len(x) * B]
    return y.reshape(len(x), B)


@pytest.mark.parametrize("N", [8, 9, 10, 11, 13, 32])
@pytest.mark.parametrize("delay", [0, 1, 2])
def test_long_window_is_the_linear_convolution(N, delay):
    B = 16
    rng = np.random.default_rng(N * 7 + delay)
    h = rng.standard_normal(N * B)
    x = list(rng.standard_normal((N + 6, B)))
    q_end = N - delay                           # a delayed filter keeps min(P, N - delay) partitions
    H = std_spectra(h, B, N)
    G = from_std(H, B, q_end)
    got = run_long(x, B, lambda t: G, delay)
    want = direct(x, h[:q_end * B], B, delay)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("N", [8, 11, 13])
def test_derivation_from_standard_spectra_matches_taps(N):
    B = 32
    h = np.random.default_rng(N).standard_normal(N * B)
    for q_end in (N, N - 1, N - 2):
        a, b = from_std(std_spectra(h, B, N), B, q_end), from_taps(h, B, q_end)
        assert [q for q, _ in a] == [q for q, _ in b]
        for (_, ga), (_, gb) in zip(a, b):
            assert np.abs(ga - gb).max() <= 1e-14


def test_no_window_reaches_beyond_n_blocks():
    """the oldest block any long partition reads is x_(t - q_end): the standard scheme's reach"""
    for N in range(8, 40):
        for q0, own in long_layout(N):
            assert q0 + 3 <= N and own <= q0 + 2 and own >= q0
        covered = sorted(q for q0, own in long_layout(N) for q in range(q0, q0 + 3) if own <= q < N)
        assert covered == list(range(N))


def test_coefficient_switch_acts_on_the_stored_history():
    """a switch at block s: from s on, the new filter over the whole input history (the standard
    scheme's meaning: the rings hold the input, the coefficients are swapped)"""
    B, N, s = 16, 11, 14
    rng = np.random.default_rng(3)
    h0, h1 = rng.standard_normal(N * B), rng.standard_normal(N * B)
    x = list(rng.standard_normal((24, B)))
    G0, G1 = from_std(std_spectra(h0, B, N), B, N), from_std(std_spectra(h1, B, N), B, N)
    got = run_long(x, B, lambda t: G0 if t < s else G1, 0)
    want = np.concatenate([direct(x, h0, B, 0)[:s], direct(x, h1, B, 0)[s:]])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_partial_last_partition_and_padding():
    """N = 11: 4 long partitions, the last aligned to the end holds 2 standard partitions of its own
    (the taps of partition 8 appear once, in partition 2)"""
    assert long_layout(11) == [(0, 0), (3, 3), (6, 6), (8, 9)]
    assert long_layout(32)[-1] == (29, 30) and len(long_layout(32)) == 11
