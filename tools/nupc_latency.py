#!/usr/bin/env python3
"""Per-period time of the non-uniform partitioned convolver on BASELINE.json configs[4]
(2-in/2-out, 1 048 576-tap room correction, float64, low-latency first block).

The I/O delay of the convolver is one period of L0 frames; what has to hold for real-time use
is that EVERY period, including the ones in which the long segments are due, is processed in
less than its duration.  Prints one JSON line: median / p99 / max milliseconds per
bfhip_nupc_block call (host buffers in and out) against the period at 48 kHz, next to the
uniform engine's block time and I/O delay for the same filters.

    python3 tools/nupc_latency.py [L0 [steps]] [--out-format S24_4LE] [--dither] [--delay] [--subdelay]
                                  [--gain-ramp] [--rewrite | --rewrite-sync | --eq [--eq-mode minimum] [--eq-taps R]
                                   | --eq-base [--eq-mode minimum] [--eq-taps R] | --eq-group [--eq-mode minimum] [--eq-taps R]]
                                  [--biquads [--biquad-phase own|linear]] [--limiter [--lookahead D] [--true-peak]] [--loudness]
                                  [--dump-output FILE] [--layout {interleaved,planar}]

--out-format sets the output sample format (default FLOAT64_LE); --dither enables HP-TPDF dither
on both outputs (an integer --out-format is needed; sample rate 48000); --delay gives both
outputs a maxdelay of 48 000 frames and new delays (seeded, up to 48 000) every 300 periods;
--subdelay gives both inputs and both outputs a sub-sample delay filter (sdf_length 31) and new
values (seeded, in (-100, 100)) every 300 periods.  --rewrite gives every filter a second set and,
every 300 periods, rewrites the idle set of each of the four filters asynchronously out of the
staging buffer (bfhip_nupc_update_coeff_async), one after the other as busy clears, then switches
to them; --rewrite-sync does the same with the synchronous bfhip_nupc_update_coeff.  Both report
the host duration of each rewrite call, the periods from call to busy == 0, and step_ms split into
periods with a rewrite in flight and without.  --eq is --rewrite with the taps rendered on the device:
every 300 periods a new random equaliser curve (130 bands, +-12 dB) is rendered at 1 048 576 taps into
the idle set of each filter (bfhip_nupc_render_eq_async), then switched to; it also reports the wall time
of synchronous renders (bfhip_nupc_render_eq: call, render, copy to the host, wait) of 8, of 16 384 and of
1 048 576 taps, made before the timed loop: an upper bound of the render's device time.  --eq-mode minimum
renders every curve with minimum phase (BFHIP_EQ_MINIMUM: no taps / 2 frames of delay; three transforms
instead of one).  --eq-taps sets the render length (default 1 048 576).  --eq-base is --eq with every curve
rendered ONTO the filter's base impulse response (bfhip_nupc_render_eq_base_async: --eq-taps taps, default
8192, above 8192 with bfhip_nupc_reserve_eq_base_long and through the big FFT, convolved with the filter's own 1 048 576 taps on the device, all partitions rewritten); its
synchronous renders are bfhip_nupc_render_eq_base at 8 and at --eq-taps taps (1 048 576 reals to the host
each).  --eq with the same --eq-taps is the plain render to hold it against.  --eq-group is the --eq-base
round with all four filters in ONE call (bfhip_nupc_render_eq_group_async: one curve per round, every filter
onto its own base); it reports what --eq-base reports.  Both report knob_to_switch: periods and frames from the
first render call of a round to the block call that commits the switch.  --biquads, with --eq, --eq-base or
--eq-group, gives every curve of the same rotation as a cascade of 32 second-order sections (a low shelf, a
high shelf and 30 peaks, +-12 dB, seeded; bfhip_nupc_render_biquads*: the sections' own phase, or
--biquad-phase linear) and reports what those options report.  --gain-ramp sets an
output gain ramp of 5 periods (bfhip_nupc_set_gain_ramp) and gives both outputs a new target (seeded,
0 .. 2) every 300 periods; it reports step_ms split into periods with a ramp in progress and without.
--limiter enables the look-ahead peak limiter (bfhip_nupc_enable_limiter: look-ahead 64 frames or --lookahead, release
4800 frames) with one group over both outputs at a threshold of 0.5; the first third of the run is 12x
louder (output peaks near 1.0), so the group limits there and idles once the filters' tail has decayed; it
reports the smallest gain the meter saw.  --true-peak (with --limiter) selects the true-peak detector
(bfhip_nupc_set_limiter_detector) and also reports the true-peak meter's reading over the run.
--loudness enables the BS.1770 loudness meter (bfhip_nupc_enable_loudness: 48 kHz, one hour of history) with one
stereo group on outputs 0, 1 -- one more launch per period -- and reports its three read-outs at the end of the run;
the limiter flags stay usable beside it.
--dump-output writes the raw output of all timed
and untimed periods to FILE (to compare two builds byte for byte).  --layout planar declares both
sides as one non-interleaved device (a plane per channel, bfhip_nupc_set_buffer_bytes): the input
period is staged and converted into the ring of reals by one more launch per period; the input
samples are the interleaved run's, plane by plane."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import brutefir_amd as bf
    ap = argparse.ArgumentParser()
    ap.add_argument("L0", nargs="?", type=int, default=64)
    ap.add_argument("steps", nargs="?", type=int, default=4096)
    ap.add_argument("--out-format", default="FLOAT64_LE")
    ap.add_argument("--dither", action="store_true")
    ap.add_argument("--delay", action="store_true")
    ap.add_argument("--subdelay", action="store_true")
    ap.add_argument("--gain-ramp", action="store_true")
    ap.add_argument("--rewrite", action="store_true")
    ap.add_argument("--rewrite-sync", action="store_true")
    ap.add_argument("--eq", action="store_true")
    ap.add_argument("--eq-mode", choices=["linear", "minimum"], default="linear")
    ap.add_argument("--eq-base", action="store_true")
    ap.add_argument("--eq-group", action="store_true")
    ap.add_argument("--eq-taps", type=int)
    ap.add_argument("--biquads", action="store_true")
    ap.add_argument("--biquad-phase", choices=["own", "linear"], default="own")
    ap.add_argument("--limiter", action="store_true")
    ap.add_argument("--lookahead", type=int, default=64)
    ap.add_argument("--true-peak", action="store_true")
    ap.add_argument("--loudness", action="store_true")
    ap.add_argument("--dump-output")
    ap.add_argument("--layout", choices=["interleaved", "planar"], default="interleaved")
    a = ap.parse_args()
    L0, steps = a.L0, a.steps
    seg_len, k = [], L0
    while k < 8192:
        seg_len.append(k)
        k *= 2
    seg_blk = [2] * len(seg_len)
    covered = 2 * sum(seg_len)
    seg_len.append(8192)
    seg_blk.append(-(-(1048576 - covered) // 8192))
    nu = bf.Nupc(seg_len, seg_blk, 8, 2, 2)
    if a.layout == "planar":
        for io, name in ((bf.IN, "FLOAT64_LE"), (bf.OUT, a.out_format)):
            fmts, n_bytes = bf.period_layout(L0, [(name, 2, [0, 1], False)])
            for c, f in enumerate(fmts):
                nu.set_format(io, c, f)
            nu.set_buffer_bytes(io, n_bytes)
    else:
        nu.set_interleaved(0, "FLOAT64_LE")
        nu.set_interleaved(1, a.out_format)
    if a.dither:
        nu.enable_dither([0, 1], 48000)
    if a.delay:
        for o in range(2):
            nu.set_maxdelay(bf.OUT, o, 48000)
            nu.set_delay(bf.OUT, o, 1000 * (o + 1))
    if a.subdelay:
        nu.enable_subdelay(31)
        for io in (bf.IN, bf.OUT):
            for c in range(2):
                nu.set_subdelay(io, c, 37 - 62 * c)
    assert a.rewrite + a.rewrite_sync + a.eq + a.eq_base + a.eq_group <= 1
    a.eq_base = a.eq_base or a.eq_group
    a.eq = a.eq or a.eq_base
    assert a.eq or (a.eq_mode == "linear" and a.eq_taps is None and not a.biquads)
    assert a.biquads or a.biquad_phase == "own"
    assert not (a.biquads and a.eq_mode == "minimum"), "sections have no homomorphic mode: their own phase is --biquad-phase own"
    eq_taps = a.eq_taps or (8192 if a.eq_base else 1048576)
    rewriting = a.rewrite or a.rewrite_sync or a.eq
    if a.rewrite or a.eq:
        nu.reserve_update()
    if a.eq:
        nu.reserve_eq(1048576)
        if a.eq_mode == "minimum":
            nu.reserve_eq_minimum()
        if a.eq_base and eq_taps > 8192:
            nu.reserve_eq_base_long()
        if a.eq_group:
            nu.reserve_eq_group(4)
    if a.limiter:
        nu.enable_limiter(a.lookahead, 4800.0)
        if a.true_peak:
            nu.set_limiter_detector(bf.LIMIT_TRUE_PEAK)
        nu.add_limiter_group([0, 1], 0.5)
    if a.loudness:
        nu.enable_loudness(48000, 36000)
        nu.add_loudness_group([0, 1])
    rng = np.random.default_rng(5)
    for o in range(2):
        for i in range(2):
            h = rng.standard_normal(1048576) * np.exp(-np.arange(1048576) / 2e5) / 2000.0
            nu.add_filter(i, o, h)
            if rewriting:
                nu.add_coeff(2 * o + i, h[:nu.taps] * 0.5)
            if a.eq_base:
                nu.reserve_eq_base(2 * o + i)
    nu.finalize()
    # two impulse responses to render alternately into the idle set (a render costs what it costs
    # the caller: here one numpy copy into the staging buffer, or nothing for the synchronous call)
    renders = [rng.standard_normal(nu.taps) * np.exp(-np.arange(nu.taps) / 2e5) / 2000.0 for _ in range(2)] if rewriting else []
    staging = nu.update_buffer() if a.rewrite else None

    def curve():
        freq = np.concatenate([[0.0], np.sort(rng.uniform(0.0005, 0.4995, 128)), [0.5]])
        return list(freq), list(10.0 ** (rng.uniform(-12, 12, 130) / 20) / 2000.0), list(rng.uniform(-3, 3, 130))


    def sections():
        s = [bf.biquad_design(bf.BIQUAD_LOW_SHELF, float(rng.uniform(0.001, 0.01)), float(rng.uniform(-12, 12)), 0.707),
             bf.biquad_design(bf.BIQUAD_HIGH_SHELF, float(rng.uniform(0.1, 0.3)), float(rng.uniform(-12, 12)), 0.707)]
        for _ in range(30):
            s.append(bf.biquad_design(bf.BIQUAD_PEAK, float(np.exp(rng.uniform(np.log(0.0005), np.log(0.45)))),
                                      float(rng.uniform(-12, 12)), float(rng.uniform(0.5, 8.0))))
        s = np.array(s)
        s[0, :3] /= 2000.0                                         # the band curves' level
        return s
    if a.biquads:
        # the curve is (sections, phase) and every render call its section counterpart
        curve = lambda: (sections(), a.biquad_phase)
        kw = {}
        render, render_async = nu.render_biquads, nu.render_biquads_async
        render_base, render_base_async, render_group_async = nu.render_biquads_base, nu.render_biquads_base_async, nu.render_biquads_group_async
    else:
        kw = {"mode": a.eq_mode}
        render, render_async = nu.render_eq, nu.render_eq_async
        render_base, render_base_async, render_group_async = nu.render_eq_base, nu.render_eq_base_async, nu.render_eq_group_async
    render_ms = []
    if a.eq:
        # a synchronous render of 8 taps is the call, the wait and a copy of 64 bytes; one of 1 048 576
        # taps adds the long render and 8 MB of copy to pageable memory
        c = curve()
        sync_taps = (8, eq_taps) if a.eq_base else (8, 16384, 1048576)
        for n_taps in sync_taps:
            for _ in range(5):
                t0 = time.perf_counter()
                if a.eq_base:
                    render_base(0, n_taps, *c, **kw)
                else:
                    render(n_taps, *c, **kw)
                render_ms.append((n_taps, (time.perf_counter() - t0) * 1e3))
    live_set, todo, round_no, due = 0, [], 0, False
    call_ms, call_copy_ms, busy_periods, started_at = [], [], [], None
    knob_at, knob_periods = None, []   # the period of a round's first render call -> periods to the committing block call
    in_flight = []                     # per period: a rewrite was in flight (or made) during it
    dump = []
    x = rng.standard_normal((8, L0, 2)) * 0.1
    if a.layout == "planar":
        x = np.ascontiguousarray(x.transpose(0, 2, 1))             # [2][L0]: a plane per channel
    x_loud, loud_until = x * 12.0, (steps + 256) // 3 if a.limiter else 0      # drives the group into limiting
    import gc
    gc.disable()                       # the timed loop allocates one small array per period
    ts = []
    drng = np.random.default_rng(9)
    n_changes = n_sd_changes = n_ramps = 0
    ramp_periods, ramp_left, ramping = 5, 0, []
    if a.gain_ramp:
        nu.set_gain_ramp(ramp_periods * L0)
    for s in range(steps + 256):
        if a.gain_ramp and s % 300 == 299:
            for o in range(2):
                nu.set_output_gain(o, float(drng.uniform(0.0, 2.0)))
            n_ramps, ramp_left = n_ramps + 1, ramp_periods
        ramping.append(ramp_left > 0)
        ramp_left = max(ramp_left - 1, 0)
        if a.delay and s % 300 == 299:
            for o in range(2):
                nu.set_delay(bf.OUT, o, int(drng.integers(0, 48001)))
            n_changes += 1
        if a.subdelay and s % 300 == 299:
            for io in (bf.IN, bf.OUT):
                for c in range(2):
                    nu.set_subdelay(io, c, int(drng.integers(-99, 100)))
            n_sd_changes += 1
        flying = False
        if rewriting:
            due = due or s % 300 == 299
            if due and not todo and started_at is None and not nu.switch_busy():
                todo, due = [0, 1, 2, 3], False
                round_no += 1
            if started_at is not None and not nu.update_busy():
                busy_periods.append(s - started_at)
                started_at = None
                assert nu.update_result() == 0
                if not todo:                                   # all four are in: switch to them
                    for f in range(4):
                        nu.set_coeff(f, 1 - live_set)
                    live_set = 1 - live_set
                    if knob_at is not None:                    # this period's block call commits the switch
                        knob_periods.append(s - knob_at)
                        knob_at = None
            if todo and started_at is None:
                f = todo.pop(0)
                if a.eq_group:
                    f, todo = [f] + todo, []
                if a.eq_base and knob_at is None:
                    knob_at = s
                src = renders[round_no & 1]
                if a.eq:
                    c = curve()
                    t0 = time.perf_counter()
                    if a.eq_group:
                        render_group_async(f, [1 - live_set] * 4, [1] * 4, eq_taps, *c, **kw)
                    elif a.eq_base:
                        render_base_async(f, 1 - live_set, eq_taps, *c, **kw)
                    else:
                        render_async(f, 1 - live_set, eq_taps, *c, **kw)
                    call_ms.append((time.perf_counter() - t0) * 1e3)
                    started_at = s
                elif a.rewrite:
                    # even rounds render into the staging buffer outside the timed call (zero-copy),
                    # odd rounds hand in a separate array (one memcpy inside the call)
                    zero_copy = round_no % 2 == 0
                    if zero_copy:
                        staging[:] = src
                    t0 = time.perf_counter()
                    nu.update_coeff_async(f, 1 - live_set, staging if zero_copy else src)
                    (call_ms if zero_copy else call_copy_ms).append((time.perf_counter() - t0) * 1e3)
                    started_at = s
                else:
                    t0 = time.perf_counter()
                    nu.update_coeff(f, 1 - live_set, src)
                    call_ms.append((time.perf_counter() - t0) * 1e3)
                    if not todo:
                        for g in range(4):
                            nu.set_coeff(g, 1 - live_set)
                        live_set = 1 - live_set
                flying = True
            flying = flying or started_at is not None
        in_flight.append(flying)
        t0 = time.perf_counter()
        st, raw = nu.block((x_loud if s < loud_until else x)[s & 7])
        ts.append(time.perf_counter() - t0)
        assert st == 0
        if a.dump_output:
            dump.append(raw)
    if a.dump_output:
        np.concatenate(dump).tofile(a.dump_output)
    ts = np.array(ts[256:]) * 1e3
    fl = np.array(in_flight[256:], bool)
    rp = np.array(ramping[256:], bool)

    def loudness_report(nu):
        r = nu.loudness(0)
        lufs = lambda v: round(v, 3) if np.isfinite(v) else None
        return {"sample_rate": 48000, "history_subblocks": 36000, "groups": [[0, 1]], "momentary_lufs": lufs(r.momentary),
                "short_term_lufs": lufs(r.short_term), "integrated_lufs": lufs(r.integrated), "subblocks": r.subblocks}

    def dist(v):
        v = np.asarray(v, float)
        if len(v) == 0:
            return None
        return {"n": int(len(v)), "median": round(float(np.median(v)), 4), "p99": round(float(np.percentile(v, 99)), 4),
                "p99.9": round(float(np.percentile(v, 99.9)), 4), "max": round(float(v.max()), 4)}
    # the periods in which every segment has a block to launch (the schedule's worst case), as
    # opposed to the rare host-side hiccups that land anywhere
    ratio = seg_len[-1] // L0
    full = ts[[i for i in range(len(ts)) if (i + 256 + 1) % ratio == 0]]
    print(json.dumps({
        "workload": "configs[4]: 2-in/2-out, %d taps, float64, partitions %s x %s" % (nu.taps, seg_len, seg_blk),
        "layout": a.layout, "out_format": a.out_format, "dithered_outputs": [0, 1] if a.dither else [],
        "delayed_outputs": {"maxdelay": 48000, "changes_every_periods": 300, "changes": n_changes} if a.delay else None,
        "subdelay": {"sdf_length": 31, "inputs": [0, 1], "outputs": [0, 1], "changes_every_periods": 300,
                     "changes": n_sd_changes} if a.subdelay else None,
        "gain_ramp": {"ramp_frames": ramp_periods * L0, "outputs": [0, 1], "new_target_every_periods": 300,
                      "ramps": n_ramps, "step_ms_ramp_in_progress": dist(ts[rp]),
                      "step_ms_no_ramp": dist(ts[~rp])} if a.gain_ramp else None,
        "rewrite": {"mode": ("eq-group" if a.eq_group else "eq-base" if a.eq_base else "eq") + ("" if a.eq_mode == "linear" else "-minimum") + ("-biquads-" + a.biquad_phase if a.biquads else "") if a.eq else "async" if a.rewrite else "sync", "every_periods": 300, "sets_per_round": 4,
                    "taps_per_set": int(nu.taps), "eq_taps": eq_taps if a.eq else None, "rounds": round_no,
                    "call_ms": dist(call_ms), "call_with_staging_copy_ms": dist(call_copy_ms),
                    "periods_to_idle": dist(busy_periods),
                    "knob_to_switch_periods": dist(knob_periods) if a.eq_base else None,
                    "knob_to_switch_frames": dist(np.array(knob_periods) * L0) if a.eq_base else None,
                    "render_eq_sync_ms": {str(k): dist([v for n_taps, v in render_ms if n_taps == k][1:])
                                          for k in sync_taps} if a.eq else None,
                    "step_ms_rewrite_in_flight": dist(ts[fl]), "step_ms_no_rewrite": dist(ts[~fl])} if rewriting else None,
        "limiter": {"lookahead_frames": a.lookahead, "release_frames": 4800, "groups": [[0, 1]], "threshold": 0.5, "loud_periods": loud_until,
                    "min_gain": round(nu.limiter_reduction(0), 4), "detector": "true_peak" if a.true_peak else "sample_peak",
                    "true_peak": round(nu.limiter_true_peak(0), 4) if a.true_peak else None} if a.limiter else None,
        "loudness": loudness_report(nu) if a.loudness else None,
        "io_delay_frames": L0, "period_ms_at_48k": L0 / 48.0,
        "step_ms": {"median": round(float(np.median(ts)), 4), "p99": round(float(np.percentile(ts, 99)), 4),
                    "p99.9": round(float(np.percentile(ts, 99.9)), 4), "max": round(float(ts.max()), 4)},
        "all_segments_due_ms": {"periods": int(len(full)), "median": round(float(np.median(full)), 4),
                                "max": round(float(full.max()), 4)},
        "slowest_periods": [[int(i) + 256, round(float(ts[i]), 3)] for i in np.argsort(ts)[::-1][:4]],
        "realtime_margin_p99.9": round(float(L0 / 48.0 / np.percentile(ts, 99.9)), 2),
        "realtime_margin_max": round(float(L0 / 48.0 / ts.max()), 2),
        "uniform_engine_io_delay_frames": 8192, "steps": steps}), flush=True)


if __name__ == "__main__":
    main()
