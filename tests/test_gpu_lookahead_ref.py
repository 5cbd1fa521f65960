"""The look-ahead long-window MAC (kernels.h: mac_la_kernel -- la_head_phase, la_tail_phase, la_far_phase;
passes.hip: the validity tables; plan.hip: long_gates) held to the float64 crossbar model
(tests/xbar_ref.py), next to the standard plan run on the same blocks.

Every case builds its engines from one rig (tests/long_rig.py): the plan under test ("la": one tier,
"far": two tiers) and the standard plan, float32, L = 8192, S24_4LE in, FLOAT_LE out.  The impulse
responses are FLAT (white noise of unit energy, one per (output, input) pair): the far tier then carries
67 % of the output amplitude at N = 11 and the shifted last partition 52 % (3.8 % and 1.25 % with the
decaying responses of the other look-ahead tests), so that an error of 1e-3 in one far partition stands
far above the limits.  Both engines are held to the model: within TOL_BLOCK relative RMS on every block
and TOL_RUN over the run, a silent block exactly silent.  Every case asserts on every block the tier it
means to reach (lookahead_blocks, lookahead_far_blocks, window_blocks) and from mac_counts the launch
kind: the head pass, one launch per block, in steady state; the full long MAC (two launches) for six
(one tier: three) blocks after an event.  One "LAREF <case> plan=... worst_block=... worst_run=..."
line per case and plan.

    a  shapes from a cold start, N + 12 blocks: every last-partition shift, slices with and without
       entries, two output groups, the 11 long partitions of config C; N = 8 under "far" (the far gate
       refuses -- three long partitions, the shifted last one reaches block t - 5 --, the near tier runs);
       sets of 9 L + 1 taps
    b  impulse probes at every t mod 6: the outputs carry the input's taps and nothing else, within NOISE
    c  per-input delays up to the clamp: entries of one long partition (no tail; the head pass reads the
       shifted window), of two (near, no far) between tailed ones, a far slice without far partitions
    d  events at every t mod 6: rewrites of the head, near, far and shifted last partitions; set_coeff
       hard and cross-faded, set_scale and set_delayblocks (private rings: standard blocks from there on,
       the model follows the ring); real-time intervals (no look-ahead inside; what was stored before must
       not reach an output after); prewarm (a second call after blocks have run is refused, BFHIP_ESTATE,
       and changes nothing)
    e  element 0: DC and Nyquist tones, from block 0 and from a block with t mod 6 = 2

Limits.  TOL_BLOCK = 2e-5 and TOL_RUN = 1e-5 are test_gpu_long_window_ref.py's; NOISE starts from
test_gpu_xbar_shapes.NOISE[4] = 4e-7 ||h||_2 and is the larger of that and twice the worse of the plain
long plan and the standard plan on the same probes.  Measured on an MI355X (worst over the file):

    standard plan   3.24e-7 per block, 3.16e-7 over a run (16 x 8 at N = 32; 3.0e-7 at N <= 20): within
                    the existing limits, so they hold for the look-ahead plans unchanged
    "la"            4.51e-7 per block, 4.40e-7 over a run (16 x 8 at N = 32; 4.2e-7 elsewhere)
    "far"           4.33e-7 per block, 4.25e-7 over a run; element 0 alone (a tone): 6.36e-7 per block
                    (standard plan there: 3.41e-7)
    probe noise     standard plan 4.9e-9, plain long plan 7.6e-9, "la" and "far" 7.6e-9 of ||h||_2: twice
                    the worse is 1.5e-8, so NOISE stays at 4e-7
"""
import numpy as np
import pytest

import brutefir_amd as bf
from long_rig import L, TOL_BLOCK, TOL_RUN, Rig, blocks_for, drive, errors, flat_ir, hold

pytestmark = pytest.mark.gpu
NOISE = 4e-7
LAG = {"la": 3, "far": 6}                    # blocks of full long MAC before the head pass is back
TIER = {"std": (2, 0, 0), "long": (4, 0, 0), "la": (4, 3, 0), "far": (4, 3, 6)}

_shared = {}


def shared(key, make):
    """what two cases on the same inputs share (the model's output, the standard engine's run): made
    once, kept until another key asks"""
    if key is None:
        return make()
    if _shared.get("key") != key:
        _shared.clear()
        _shared.update(key=key, val=make())
    return _shared["val"]


def run_plan(monkeypatch, rig, plan, blocks, actions=None, rt=None, before=None):
    e = rig.engine(monkeypatch, plan)
    try:
        r = drive(rig, e, blocks, actions, rt, before)
    finally:
        e.close()
    assert r.sts == [0] * len(blocks), (plan, r.sts)
    return r


def steady(r, plan, tier=None, first=None):
    """the tier on every block, and from block `first` on the head pass alone: one launch per block"""
    n = len(r.sts)
    w, a, f = TIER[tier or plan]
    assert r.wins == [w] * n and r.la == [a] * n and r.far == [f] * n, (plan, r.wins, r.la, r.far)
    launches, heads, fulls = zip(*r.counts)
    if not a:
        assert heads[-1] == 0 and fulls[-1] == 0, r.counts[-1]
        return
    first = (6 if f else 3) if first is None else first
    assert heads[-1] + fulls[-1] == n and fulls[-1] <= first and launches[-1] == heads[-1] + 2 * fulls[-1], r.counts[-1]
    assert n > first + 3
    assert [heads[k] - heads[k - 1] for k in range(first, n)] == [1] * (n - first), r.counts
    assert [launches[k] - launches[k - 1] for k in range(first, n)] == [1] * (n - first), r.counts


def case(monkeypatch, name, rig, blocks, plan, tiers=steady, actions=None, rt=None, before=None, share=None,
         tol=(TOL_BLOCK, TOL_RUN), skip=0):
    """the plan under test and the standard plan on the same blocks, both held to the model (but for the
    first `skip` blocks, silent ones, where the model leaves its own rounding: those to exact silence)"""
    sets = dict(rig.sets)                    # (the model's rewrites replace entries: engines start from these)

    def reference():
        s = run_plan(monkeypatch, rig, "std", blocks, actions, rt, before)
        return rig.expect(blocks, actions), s
    want, s = shared(share, reference)
    rig.sets = sets
    r = run_plan(monkeypatch, rig, plan, blocks, actions, rt, before)
    assert not np.any(r.y[:skip * L]) and not np.any(s.y[:skip * L])     # silent blocks in, silent blocks out
    want, r, s = want[skip * L:], r._replace(y=r.y[skip * L:]), s._replace(y=s.y[skip * L:])
    for p, res in ((plan, r), ("std", s)):
        print("LAREF %s plan=%s worst_block=%.3g worst_run=%.3g" % ((name, p) + errors(res.y, want)))
    tiers(r, plan)
    n = len(blocks)
    assert s.wins == [2] * n and s.la == [0] * n and s.far == [0] * n and s.counts[-1][1:] == (0, 0)
    hold(r.y, want, name + " " + plan, *tol)
    hold(s.y, want, name + " std", *tol)
    return r, s, want


# ------------------------------------------------------------------ a. shapes

SHAPES = [(8, 8, 9), (8, 8, 10), (8, 8, 11), (8, 8, 13), (8, 8, 20), (3, 8, 11), (1, 8, 20), (5, 16, 13), (8, 16, 11),
          (16, 8, 32)]


@pytest.mark.parametrize("I,O,N,plan", [s + (p,) for s in SHAPES for p in ("la", "far")])
def test_shapes_from_a_cold_start(monkeypatch, I, O, N, plan):
    """N + 12 blocks: zeroed ahead buffers, warm-up (the blocks ahead have more partitions than the block
    itself: the guarded loops), steady state.  (8, 8): shifts 0, 2, 1, 2, 1 at N = 9, 10, 11, 13, 20;
    (3, 8): far slices 1/1/1/0/0/0; (1, 8): near 1/0/0, far 1/0/0/0/0/0; (5, 16) and (8, 16): two groups;
    (16, 8) at N = 32: 11 long partitions, near slices 6/5/5, far 3/3/3/3/2/2"""
    rig = Rig(N, I, O, seed=100 * N + I, ir="flat")
    case(monkeypatch, "a %dx%d N=%d" % (I, O, N), rig, blocks_for(rig, N + 12), plan, share=("a", I, O, N))


def test_shape_far_gate_refuses_three_partitions(monkeypatch):
    """N = 8 under "far": three long partitions, the last shifted by one block -- it reads block t - 5,
    which a call six blocks earlier does not have.  The far gate refuses, the near tier runs"""
    rig = Rig(8, 8, 8, seed=808, ir="flat")
    case(monkeypatch, "a 8x8 N=8 far-refused", rig, blocks_for(rig, 20), "far",
         tiers=lambda r, plan: steady(r, plan, tier="la"))


@pytest.mark.parametrize("plan", ["la", "far"])
def test_shape_sets_one_tap_into_their_last_partition(monkeypatch, plan):
    """all sets 9 L + 1 taps at N = 12: ten standard partitions, the last one a single tap; four long
    partitions, the last shifted by two blocks"""
    N, I, O = 12, 8, 8
    rig = Rig(N, I, O, seed=1212, ir="flat", lengths={(o, i): 9 * L + 1 for o in range(O) for i in range(I)})
    case(monkeypatch, "a 8x8 N=12 taps=9L+1", rig, blocks_for(rig, N + 12), plan, share=("a9", N))


# ------------------------------------------------------------------ b. impulse probes

_probe_rig = {}


def probe_rig(N, I, O):
    """one set of responses for every probe: built once"""
    if (N, I, O) not in _probe_rig:
        _probe_rig.clear()
        _probe_rig[(N, I, O)] = Rig(N, I, O, seed=2000, ir="flat")
    return _probe_rig[(N, I, O)]


def probe(monkeypatch, plan, rig, b0, frame, inputs, amp=0.5):
    """an impulse of `amp` (exact in S24) on `inputs` at `frame` of block b0, N + 1 blocks further ->
    (max |error| / (amp ||h||_2) per output, Run)"""
    N, I, O = rig.N, rig.I, rig.O
    n_blocks = b0 + N + 2
    x = np.zeros((n_blocks * L, I), np.int32)
    t0 = b0 * L + frame
    for i in inputs:
        x[t0, i] = int(amp * (1 << 23))
    blocks = [np.ascontiguousarray(x[b * L:(b + 1) * L]) for b in range(n_blocks)]
    r = run_plan(monkeypatch, rig, plan, blocks)
    want = np.zeros((n_blocks * L, O))
    for o in range(O):
        for i in inputs:
            h = rig.sets[(o, i)]
            m = min(len(h), len(want) - t0)
            want[t0:t0 + m, o] += amp * h[:m]
    norm = amp * max(np.sqrt((rig.sets[(o, i)] ** 2).sum()) for o in range(O) for i in inputs)
    return np.abs(r.y - want).max(axis=0) / norm, r


PROBES = [(b0, 0, (b0 % 8,)) for b0 in range(6, 12)] + [(8, L - 1, (3,)), (9, 0, (1, 6))]


@pytest.mark.parametrize("b0,frame,inputs", PROBES, ids=["b%d-f%d-i%s" % (b, f, "+".join(map(str, i))) for b, f, i in PROBES])
def test_impulse_probes(monkeypatch, b0, frame, inputs):
    """(8, 8), N = 20, "far": the head pass is in steady state from block 6 on, so b0 = 6 .. 11 puts the
    impulse, and with it every partition of the response over the N + 1 blocks after, at every value of
    t mod 6 and t mod 3; once at the last frame of a block, once on two inputs of different far slices
    (2/2/1/1/1/1: inputs 1 and 6).  Every output sample -- the taps, the blocks before the impulse, the
    frames after the response's end, nothing from the seven other inputs' sets -- within NOISE ||h||_2"""
    rig = probe_rig(20, 8, 8)
    res = {}
    for plan in ("far", "std"):
        err, r = probe(monkeypatch, plan, rig, b0, frame, inputs)
        print("LAREF b b0=%d frame=%d inputs=%s plan=%s err/|h|=%.3g" % (b0, frame, inputs, plan, err.max()))
        steady(r, plan)
        assert not np.any(r.y[:b0 * L]), plan                  # silent blocks in, silent blocks out: exactly
        res[plan] = err
    for plan, err in res.items():
        assert err.max() <= NOISE, (plan, err)


# ------------------------------------------------------------------ c. delays

@pytest.mark.parametrize("N,plan", [(N, p) for N in (11, 12) for p in ("la", "far")])
def test_delays_up_to_the_clamp(monkeypatch, N, plan):
    """per-input delays 0, N - 1, 1, N - 3, 5, 2, N + 4 (clamped to N - 1), 0.  With full-length sets
    every entry passes both gates (3 (P - 1) - shift + delay = N - 3 for every delay).  Inputs 1, 3 and 6
    have one long partition: no tail, and their head reads the shifted window; input 4 at N = 11 has two:
    near, no far.  The entries without tails sit between tailed ones in near slice 0 (0 1 2 | 3 4 5 | 6 7)
    and in far slices 0 and 1 (0 1 | 2 3 | 4 | 5 | 6 | 7); far slice 4 (input 6) has no far partition and
    must store zeros"""
    d = [0, N - 1, 1, N - 3, 5, 2, N + 4, 0]
    rig = Rig(N, 8, 8, seed=31 + N, delays=dict(enumerate(d)), ir="flat")
    case(monkeypatch, "c N=%d" % N, rig, blocks_for(rig, 2 * N + 8), plan, share=("c", N))


# ------------------------------------------------------------------ d. events

def event_tiers(events, plan):
    """events: [(block, kind)] in block order, kind "bump" (stored products are void: a rewrite, a hard
    set_coeff), "fade" (the same, and the block itself runs the standard MAC), "leave" (the plan runs
    standard blocks from here on).  After a bump the full long MAC runs until the far (near) passes of six
    (three) calls have refilled a block's buffers; the next event comes only after the head pass is back"""
    def check(r, plan_):
        n = len(r.sts)
        lag = LAG[plan]
        leave = min([b for b, k in events if k == "leave"], default=n)
        fades = [b for b, k in events if k == "fade"]
        wins = [2 if (k >= leave or k in fades) else 4 for k in range(n)]
        assert r.wins == wins, r.wins
        assert r.la == [3 if w == 4 else 0 for w in wins], r.la
        assert r.far == [LAG[plan] if (w == 4 and plan == "far") else 0 for w in wins], r.far
        launches, heads, fulls = zip(*r.counts)
        head_at = [k for k in range(n) if heads[k] - (heads[k - 1] if k else 0) == 1]
        one_launch = [k for k in range(n) if launches[k] - (launches[k - 1] if k else 0) == 1]
        first = events[0][0]
        assert first > lag + 1 and all(k in head_at for k in range(lag, first)), (plan, r.counts)
        bumps = [(b, k) for b, k in events if b < leave and k != "leave"]
        for j, (b, kind) in enumerate(bumps):
            nxt = bumps[j + 1][0] if j + 1 < len(bumps) else min(leave, n)
            back = next((k for k in range(b, n) if k in head_at), n)
            assert lag <= back - b <= lag + 1 and back < nxt, (plan, b, kind, back, r.counts)
            assert fulls[back] - fulls[b - 1] == lag, (plan, b, kind, r.counts)      # the fade block: neither
            assert all(k in head_at and k in one_launch for k in range(back, nxt)), (plan, b, kind, r.counts)
        if leave < n:
            assert heads[-1] == heads[leave - 1] and fulls[-1] == fulls[leave - 1], (plan, r.counts)
    return check


def event_rig(N, seed, **kw):
    delays = dict(enumerate(int(v) for v in np.random.default_rng(5).integers(0, 3, 8)))
    return Rig(N, 8, 8, seed=seed, delays=delays, n_extra=1, ir="flat", **kw)


EVENT_CASES = [("far", ph) for ph in range(6)] + [("la", 1), ("la", 2)]


@pytest.mark.parametrize("plan,phase", EVENT_CASES)
def test_rewrites_of_every_tier(monkeypatch, plan, phase):
    """update_coeff_block on a set in use (input 2: no delay, all N partitions) at standard partitions 0 (the head partition), 3 (near tier),
    6 (far tier), 9 and 10 (the first and last block of the shifted last long partition), eight blocks
    apart from block N + 1 + phase on: the products stored ahead with the old taps must not reach an
    output, the new ones must reach every later block"""
    N = 11
    rig = event_rig(N, 4100 + phase)
    rng = np.random.default_rng(40 + phase)
    t0 = N + 1 + phase
    parts = [0, 3, 6, 9, 10]
    actions = {t0 + 8 * j: [("rewrite", (3, 2), q, flat_ir(int(rng.integers(1 << 30)), L, 8))] for j, q in enumerate(parts)}
    blocks = blocks_for(rig, t0 + 8 * len(parts) + 1)
    case(monkeypatch, "d rewrites phase=%d" % phase, rig, blocks, plan, actions=actions,
         tiers=event_tiers([(b, "bump") for b in sorted(actions)], plan))


@pytest.mark.parametrize("plan,phase", EVENT_CASES)
def test_switches_scale_and_delay(monkeypatch, plan, phase):
    """set_coeff without cross-fade (filter 3), eight blocks later with it (filter 12: that block runs
    the standard MAC, then the full long MAC, then the head pass again); nine blocks later set_scale on
    filter 9 and, three blocks on, set_delayblocks on filter 30: both filters get rings of their own, the
    plan runs standard blocks from the first of them on and the model follows the rings for N blocks"""
    N, I = 11, 8
    rig = event_rig(N, 4200 + phase, crossfade={12})
    t0 = N + 1 + phase
    actions = {t0: [("coeff", 3, ("x", 0))], t0 + 8: [("coeff", 12, ("x", 0))],
               t0 + 17: [("scale", 9, 0, 0, 0.5)], t0 + 20: [("delay", 30, 3)]}
    blocks = blocks_for(rig, t0 + 20 + N + 2)
    case(monkeypatch, "d switches phase=%d" % phase, rig, blocks, plan, actions=actions,
         tiers=event_tiers([(t0, "bump"), (t0 + 8, "fade"), (t0 + 17, "leave")], plan))


@pytest.mark.parametrize("plan,phase", EVENT_CASES)
def test_real_time_intervals(monkeypatch, plan, phase):
    """N + 2 + phase blocks, then rt_begin, four rt_block calls, rt_end, ten plain blocks; the same with
    RT_OVERLAP through rt_submit / rt_wait, ten plain blocks.  A real-time block has no tail pass: the
    head-block count stands still inside an interval (lookahead_blocks reads 0 there), what was stored
    before it must not reach a block after it, and the head pass is back within seven blocks"""
    N = 11
    rig = event_rig(N, 4300 + phase)
    a0 = N + 2 + phase
    spans = [(a0, a0 + 4, 0), (a0 + 14, a0 + 18, bf.RT_OVERLAP)]
    blocks = blocks_for(rig, a0 + 28)

    def tiers(r, plan_):
        n = len(r.sts)
        inside = [any(a <= k < z for a, z, _ in spans) for k in range(n)]
        assert r.wins == [4] * n, r.wins
        assert r.la == [0 if i else 3 for i in inside], r.la
        assert r.far == [LAG[plan] if (plan == "far" and not i) else 0 for i in inside], r.far
        launches, heads, fulls = zip(*r.counts)
        assert [heads[k] - heads[k - 1] for k in range(LAG[plan], a0)] == [1] * (a0 - LAG[plan]), r.counts
        for a, z, _ in spans:
            assert heads[z - 1] == heads[a - 1] and fulls[z - 1] == fulls[a - 1], (a, z, r.counts)
            back = next((k for k in range(z, n) if heads[k] > heads[z - 1]), n)
            assert LAG[plan] <= back - z < 7, (a, z, back, r.counts)
            assert [heads[k] - heads[k - 1] for k in range(back, z + 10)] == [1] * (z + 10 - back), r.counts
            assert [launches[k] - launches[k - 1] for k in range(back, z + 10)] == [1] * (z + 10 - back), r.counts

    case(monkeypatch, "d real-time phase=%d" % phase, rig, blocks, plan, rt=spans, tiers=tiers)


@pytest.mark.parametrize("plan", ["la", "far"])
def test_real_time_first_block(monkeypatch, plan):
    """the very first block in real-time mode, plain blocks from the second on.  The ahead buffers primed
    at the start are marked for blocks 1 and 2 as well, and only the epoch do_mac bumps for a block
    without a tail pass says that they no longer line up (everywhere else the `for` tables refuse such a
    block on their own): no head pass until the calls after the interval have refilled a block's buffers"""
    N = 11
    rig = event_rig(N, 4350)

    def tiers(r, plan_):
        n, lag = len(r.sts), LAG[plan]
        assert r.wins == [4] * n and r.la == [0] + [3] * (n - 1), (r.wins, r.la)
        launches, heads, fulls = zip(*r.counts)
        assert heads[lag] == 0 and fulls[lag] == lag, r.counts
        assert [heads[k] - heads[k - 1] for k in range(lag + 1, n)] == [1] * (n - lag - 1), r.counts

    case(monkeypatch, "d real-time first block", rig, blocks_for(rig, N + 8), plan, rt=[(0, 1, 0)], tiers=tiers)


@pytest.mark.parametrize("plan", ["la", "far"])
def test_prewarm(monkeypatch, plan):
    """prewarm() before the first block: N blocks of silence count as processed, the ahead buffers are
    primed, the head pass runs from the first block on.  A second call after N + 3 blocks is refused
    (BFHIP_ESTATE) and must leave the engine as it was: the head pass goes on, the outputs hold"""
    N = 11
    rig = event_rig(N, 4400)

    def again(e):
        with pytest.raises(bf.BfhipError):
            e.prewarm()

    case(monkeypatch, "d prewarm", rig, blocks_for(rig, N + 10), plan, before={0: lambda e: e.prewarm(), N + 3: again},
         tiers=lambda r, p: steady(r, p, first=1), share=("prewarm",))


# ------------------------------------------------------------------ e. element 0

def tone_blocks(kind, n_silent, n_blocks, I):
    """S24_4LE blocks of a constant (its spectrum is DC only) or of +c, -c, +c ... (Nyquist only), after
    n_silent blocks of zeros"""
    c = int(0.1 * (1 << 23))
    col = np.full(L, c, np.int32)
    if kind == "nyquist":
        col[1::2] = -c
    tone = np.ascontiguousarray(np.repeat(col[:, None], I, axis=1))
    return [np.zeros_like(tone)] * n_silent + [tone] * n_blocks


@pytest.mark.parametrize("start", [0, 8])
@pytest.mark.parametrize("N", [11, 20])
@pytest.mark.parametrize("kind", ["dc", "nyquist"])
def test_element_0(monkeypatch, kind, N, start):
    """a constant input excites DC alone, the alternating one Nyquist alone: both live in element 0 of the
    packed spectrum, the one product with a fix-up (one lane of one wave runs that copy of the three
    passes).  The tone from block 0, and from block 8 (t mod 6 = 2, t mod 3 = 2)"""
    rig = Rig(N, 8, 8, seed=500 + N, ir="flat")
    blocks = tone_blocks(kind, start, N + 8, 8)
    r, s, want = case(monkeypatch, "e %s N=%d start=%d" % (kind, N, start), rig, blocks, "far", skip=start)
    assert all(np.any(want[k * L:(k + 1) * L]) for k in range(len(blocks) - start))
