"""The float64 model of the BS.1770 loudness meter (include/bfhip_nupc.h), in numpy alone: the K-weighting design for
any rate, the two sections walked frame by frame in transposed direct form II, sub-block energies, the read-outs
with the gate, and a decoder from the raw bytes a convolver returned to fractions of full scale.  Held to the
standard in tests/test_loudness_model.py; the device is held to it in tests/test_gpu_nupc_loudness.py."""
import collections
import math

import numpy as np

Readout = collections.namedtuple("Readout", "momentary short_term integrated subblocks first wrapped")
NINF = float("-inf")


def kweighting(fs):
    """shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2: the bilinear redesign of the BS.1770 prototype"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(shelf + hp)


def kfilter(v, fs):
    """z of one channel, fresh state: o = b0 v + s1; s1 = b1 v - a1 o + s2; s2 = b2 v - a2 o, shelf then high-pass;
    a value that is not finite counts as 0"""
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = (float(x) for x in kweighting(fs))
    s1 = s2 = r1 = r2 = 0.0
    x = np.asarray(v, np.float64)
    x = np.where(np.isfinite(x), x, 0.0).tolist()
    z = [0.0] * len(x)
    for t, u in enumerate(x):
        o = b0 * u + s1
        s1 = b1 * u - a1 * o + s2
        s2 = b2 * u - a2 * o
        y = c0 * o + r1
        r1 = c1 * o - d1 * y + r2
        r2 = c2 * o - d2 * y
        z[t] = y
    return np.array(z)


def channel_energy(v, fs):
    """sum of z^2 over each complete sub-block of S = fs / 10 frames, one channel, weight 1"""
    S = fs // 10
    z = kfilter(v, fs)
    n = len(z) // S
    return np.array([math.fsum(z[j * S:(j + 1) * S] ** 2) for j in range(n)])


def group_energy(v, fs, weights=None):
    """E[j] of a group: v [frames][members] as fractions of full scale"""
    v = np.asarray(v, np.float64)
    w = np.ones(v.shape[1]) if weights is None else np.asarray(weights, np.float64)
    return sum(w[c] * channel_energy(v[:, c], fs) for c in range(v.shape[1]))


def lufs(m):
    return -0.691 + 10.0 * math.log10(m) if m > 0.0 else NINF


def readout(E, fs, reset=0, history=None):
    """the read-outs from E[0 .. subblocks): sub-blocks from finalize on; history: the ring's length (None: nothing
    is dropped); reset: the first sub-block the integrated value may cover"""
    S = fs // 10
    n = len(E)
    J = n - 1
    oldest = max(n - history, 0) if history else 0
    first = max(reset, oldest)
    win = lambda last, k: math.fsum(E[last - k + 1:last + 1]) / (k * S)
    mom = lufs(win(J, 4)) if n >= 4 else NINF
    short = lufs(win(J, 30)) if n >= 30 else NINF
    B = [win(j, 4) for j in range(first + 3, n)]
    B = [b for b in B if lufs(b) > -70.0]
    integ = NINF
    if B:
        rel = lufs(math.fsum(B) / len(B)) - 10.0
        B2 = [b for b in B if lufs(b) > rel]
        if B2:
            integ = lufs(math.fsum(B2) / len(B2))
    return Readout(mom, short, integ, n, first, oldest > reset)


def ungated(E, fs):
    """l of the mean square over all of E, silence included: what the gate is held against"""
    return lufs(math.fsum(E) / (len(E) * (fs // 10)))


def decode(raw, fmts, L0, period_bytes):
    """the raw output of whole periods (uint8, periods * period_bytes) -> v [frames][channels], each sample as
    load_raw reads it (by the channel's byte_offset, sample_spacing, bytes) times the format's scale"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1, period_bytes)
    out = np.zeros((raw.shape[0] * L0, len(fmts)))
    for c, f in enumerate(fmts):
        stride = f.sample_spacing * f.bytes
        idx = f.byte_offset + np.arange(L0)[:, None] * stride + np.arange(f.bytes)[None, :]
        b = raw[:, idx]                                            # [periods][L0][bytes]
        if f.swap:
            b = b[:, :, ::-1]
        b = np.ascontiguousarray(b)
        if f.isfloat:
            val = b.view("<f4" if f.bytes == 4 else "<f8")[:, :, 0].astype(np.float64)
        elif f.bytes == 3:
            u = b[:, :, 0].astype(np.int64) | b[:, :, 1].astype(np.int64) << 8 | b[:, :, 2].astype(np.int64) << 16
            val = (u - ((u & 0x800000) << 1)).astype(np.float64)
        else:
            val = b.view({1: "i1", 2: "<i2", 4: "<i4"}[f.bytes])[:, :, 0].astype(np.float64)
        out[:, c] = (val * f.scale).ravel()
    return out


def sine(fs, seconds, freq=997.0, amp=1.0):
    return amp * np.sin(2.0 * np.pi * freq * np.arange(int(round(fs * seconds))) / fs)
