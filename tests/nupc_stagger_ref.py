"""Float64 model of the non-uniform convolver's staggered switches (include/bfhip_nupc.h,
BFHIP_NUPC_SWITCH_STAGGERED), for the tests.  numpy only.

A schedule is (seg_length, seg_blocks); segment k covers taps [off_k, off_k + N_k L_k).  A request
group committed by the block call whose first output frame is t_req gives segment k the switch frame

    t_k = e_k - L_k + off_k,   e_k = the first multiple of L_k >= t_req + L0,

and the output, in front of output gain and quantisation, is

    y(t)   = sum_k [ (1 - w_k(t)) y_old,k(t) + w_k(t) y_new,k(t) ]
    w_k(t) = 0 below t_k,  (t - t_k) / (F - 1) in [t_k, t_k + F),  1 from t_k + F on  (F = 0: a step)

with y_A,k the full-history convolution of the inputs with segment k's slice of the taps under
assignment A.  Several commits apply in order, each to the result of the one before: a later switch
whose t_k equals an earlier hard switch's replaces it in that segment."""
import numpy as np


def offsets(sched):
    """first tap of every segment"""
    off, out = 0, []
    for L, N in zip(*sched):
        out.append(off)
        off += L * N
    return out


def switch_frames(sched, t_req):
    """t_k of a request group committed at t_req (a multiple of L0), by the formula"""
    L0 = sched[0][0]
    out = []
    for L, off in zip(sched[0], offsets(sched)):
        e = -(-(t_req + L0) // L) * L
        out.append(e - L + off)
    return out


def switch_frames_walk(sched, t_req):
    """the same by walking the launch grid: the block call with first output frame t has received
    t + L0 frames and launches segment k iff L_k divides that; the launch writes frames from
    t + L0 - L_k + off_k on.  t_k is the first frame written by segment k's first launch in a block
    call at or after the committing one."""
    L0 = sched[0][0]
    out = []
    for L, off in zip(sched[0], offsets(sched)):
        t = t_req
        while (t + L0) % L:
            t += L0
        out.append(t + L0 - L + off)
    return out


def weight(n, t_k, F):
    """w_k(t) for t = 0 .. n - 1"""
    t = np.arange(n)
    if F == 0:
        return (t >= t_k).astype(np.float64)
    return np.clip((t - t_k) / (F - 1.0), 0.0, 1.0) * (t >= t_k)


def slices(h, sched):
    """the taps cut into the segments' slices, each zero outside its own (their sum is h, cut or
    zero-padded to the schedule)"""
    taps = sum(L * N for L, N in zip(*sched))
    full = np.zeros(taps)
    m = min(len(h), taps)
    full[:m] = np.asarray(h, np.float64)[:m]
    out = []
    for L, N, off in zip(sched[0], sched[1], offsets(sched)):
        s = np.zeros(taps)
        s[off:off + L * N] = full[off:off + L * N]
        out.append(s)
    return out


def conv(x, h, n):
    """float64 linear convolution of x with h, first n frames"""
    x = np.asarray(x, np.float64)[:n]
    h = np.asarray(h, np.float64)
    nfft = 1 << max(len(x) + len(h) - 2, 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x, nfft) * np.fft.rfft(h, nfft), nfft)[:n]


def segment_outputs(x, filters, sched, n_out):
    """x: [frames][n_in]; filters: (in, out, taps, scale) -> [segment][frames][n_out], y_A,k of
    the assignment that these taps and scales (in * out * gain) are"""
    n = len(x)
    out = np.zeros((len(sched[0]), n, n_out))
    for i, o, h, sc in filters:
        for k, hk in enumerate(slices(h, sched)):
            out[k, :, o] += conv(x[:, i], hk, n) * sc
    return out


def staggered(yseg, commits, sched, frames=None):
    """yseg[a]: [segment][frames][n_out] under assignment a (0 is the one the run starts with);
    commits: [(t_req, F, a)] in order.  frames(t_req) -> [t_k] replaces the formula (the model
    tests force all t_k equal with it).  Returns [frames][n_out]."""
    frames = frames or (lambda t_req: switch_frames(sched, t_req))
    cur = np.array(yseg[0], np.float64)
    n = cur.shape[1]
    for t_req, F, a in commits:
        for k, t_k in enumerate(frames(t_req)):
            w = weight(n, t_k, F)[:, None]
            cur[k] = (1.0 - w) * cur[k] + w * yseg[a][k]
    return cur.sum(axis=0)


def busy_after(sched, end, t_seg, F):
    """bfhip_nupc_switch_busy after the block call that has received `end` frames: does some
    segment's next block start before the segment's own fade ends?"""
    return any(end // L * L + off < t_k + F for L, off, t_k in zip(sched[0], offsets(sched), t_seg))


SMALL = ([64, 128, 256, 512], [2, 2, 2, 6])     # offsets 0, 128, 384, 896: all but the first in the background
ZERO = ([64, 128, 256], [1, 1, 4])              # offsets 0, 64, 192: zero slack, all on the main stream


class Crossbar:
    """the data of a 2x2 crossbar (filter f = 2 * out + in) with n_sets impulse responses per filter
    over the whole schedule, flat noise, and its model.  An assignment is a list of (set, gain), one
    per filter; `set` indexes h[f], which a test may append to."""

    def __init__(self, sched, n_sets, seed, n_frames, dt=np.float64):
        self.sched, self.dt = sched, dt
        self.taps = sum(L * N for L, N in zip(*sched))
        rng = np.random.default_rng(seed)
        self.h = [[(rng.standard_normal(self.taps) / np.sqrt(self.taps)).astype(dt) for _ in range(n_sets)]
                  for _ in range(4)]
        self.in_scale = [0.5 if f % 2 else 1.0 for f in range(4)]
        self.out_scale = [-1.0 if f // 2 else 1.0 for f in range(4)]
        self.x = (rng.standard_normal((n_frames, 2)) * 0.1).astype(dt)
        self._y = {}

    def yseg(self, asg):
        """[segment][frames][2] under the assignment, float64"""
        n = len(self.x)
        out = np.zeros((len(self.sched[0]), n, 2))
        for f, (j, gain) in enumerate(asg):
            if (f, j) not in self._y:
                self._y[f, j] = segment_outputs(self.x, [(f % 2, 0, self.h[f][j], 1.0)], self.sched, 1)[:, :, 0]
            out[:, :, f // 2] += self._y[f, j] * (self.in_scale[f] * self.out_scale[f] * gain)
        return out

    def model(self, commits, start=None):
        """commits: [(t_req, F, assignment)] -> [frames][2]"""
        start = start or [(0, 1.0)] * 4
        return staggered([self.yseg(start)] + [self.yseg(a) for _, _, a in commits],
                         [(t, F, i + 1) for i, (t, F, _) in enumerate(commits)], self.sched)
