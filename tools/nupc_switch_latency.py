#!/usr/bin/env python3
"""Per-period time of the non-uniform partitioned convolver on BASELINE.json configs[4]
(2-in/2-out, 1 048 576-tap room correction, float64, 64-frame periods) while coefficient
switches run back to back: the first half of the timed periods runs without switches, then a
new switch (every filter to the other of two sets, cross-fade length L0) is queued as soon as
the last one has left bfhip_nupc_switch_busy.

Periods are split into switch-window periods (a switch is committed by the call or still in
flight when it starts: segment blocks run under both assignments, segment engines rebuild
their plans) and steady periods (no switch in flight).  Prints one JSON line: median / p99.9 /
max milliseconds per bfhip_nupc_block call for both, against the period at 48 kHz.  Compare the
steady line with tools/nupc_latency.py, which never switches.

    python3 tools/nupc_switch_latency.py [L0 [steps]] [--gain] [--staggered]

--gain: the switches are gain-only (bfhip_nupc_set_filter_gain on every filter, alternating between
two gain presets; one set per filter and bfhip_nupc_reserve_filter_gain): the same window mechanism
without a second set of coefficients.
--staggered: the switches are staggered ones (bfhip_nupc_set_switch_mode): every segment switches at
its own next launch, only the blocks that overlap a segment's own fade run twice.  In both modes the
line reports the mode, the frames from the request (the committing call's first output frame) to the
first output frame the switch changes, and the switch-window periods per switch."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    return {"periods": int(len(ts)), "median": round(float(np.median(ts)), 4),
            "p99.9": round(float(np.percentile(ts, 99.9)), 4), "max": round(float(ts.max()), 4)}


def main():
    import brutefir_amd as bf
    argv = [v for v in sys.argv[1:] if v not in ("--gain", "--staggered")]
    gain = "--gain" in sys.argv[1:]
    staggered = "--staggered" in sys.argv[1:]
    L0 = int(argv[0]) if len(argv) > 0 else 64
    steps = int(argv[1]) if len(argv) > 1 else 4096
    seg_len, k = [], L0
    while k < 8192:
        seg_len.append(k)
        k *= 2
    seg_blk = [2] * len(seg_len)
    covered = 2 * sum(seg_len)
    seg_len.append(8192)
    seg_blk.append(-(-(1048576 - covered) // 8192))
    nu = bf.Nupc(seg_len, seg_blk, 8, 2, 2)
    nu.set_interleaved(0, "FLOAT64_LE")
    nu.set_interleaved(1, "FLOAT64_LE")
    rng = np.random.default_rng(5)
    for f in range(4):
        h = [rng.standard_normal(1048576) * np.exp(-np.arange(1048576) / 2e5) / 2000.0 for _ in range(2)]
        nu.add_filter(f % 2, f // 2, h[0])
        if not gain:
            nu.add_coeff(f, h[1])
    if gain:
        nu.reserve_filter_gain()
    if staggered:
        nu.set_switch_mode(bf.SWITCH_STAGGERED)
    nu.finalize()
    presets = [[1.0, 1.0, 1.0, 1.0], [0.7, -0.4, 0.25, 1.3]]
    x = rng.standard_normal((8, L0, 2)) * 0.1
    import gc
    gc.disable()                       # the timed loop allocates one small array per period
    ts, window, target, switches, heard = [], [], 1, 0, []
    for s in range(steps + 256):
        in_window = nu.switch_busy()
        if not in_window and s >= 256 + steps // 2:
            for f in range(4):
                if gain:
                    nu.set_filter_gain(f, presets[target][f])
                else:
                    nu.set_coeff(f, target)
            target, in_window, switches = 1 - target, True, switches + 1
            requested = True
        else:
            requested = False
        t0 = time.perf_counter()
        st, _ = nu.block(x[s & 7])
        ts.append(time.perf_counter() - t0)
        if requested:
            heard.append(nu.switch_frame() - s * L0)          # outside the timed section
        window.append(in_window)
        assert st == 0
    ts = np.array(ts[256:]) * 1e3
    window = np.array(window[256:])
    print(json.dumps({
        "workload": "configs[4]: 2-in/2-out, %d taps, float64, partitions %s x %s, %s, "
                    "back-to-back switches with a %d-frame cross-fade"
                    % (nu.taps, seg_len, seg_blk, "one set per filter, gain-only" if gain else "two sets per filter", L0),
        "switch_kind": "gain" if gain else "coeff",
        "switch_mode": "staggered" if staggered else "aligned",
        "request_to_first_changed_frame": {"median": int(np.median(heard)), "max": int(max(heard))} if heard else None,
        "window_periods_per_switch": round(float(window.sum()) / max(switches, 1), 2),
        "io_delay_frames": L0, "period_ms_at_48k": L0 / 48.0, "switches": switches,
        "switch_window_ms": stats(ts[window]), "steady_ms": stats(ts[~window]),
        "slowest_periods": [[int(i) + 256, round(float(ts[i]), 3), bool(window[i])] for i in np.argsort(ts)[::-1][:4]],
        "realtime_margin_window_max": round(float(L0 / 48.0 / ts[window].max()), 2),
        "steps": steps}), flush=True)


if __name__ == "__main__":
    main()
