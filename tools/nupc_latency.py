#!/usr/bin/env python3
"""Per-period time of the non-uniform partitioned convolver on BASELINE.json configs[4]
(2-in/2-out, 1 048 576-tap room correction, float64, low-latency first block).

The I/O delay of the convolver is one period of L0 frames; what has to hold for real-time use
is that EVERY period, including the ones in which the long segments are due, is processed in
less than its duration.  Prints one JSON line: median / p99 / max milliseconds per
bfhip_nupc_block call (host buffers in and out) against the period at 48 kHz, next to the
uniform engine's block time and I/O delay for the same filters.

    python3 tools/nupc_latency.py [L0 [steps]] [--out-format S24_4LE] [--dither] [--delay] [--subdelay]

--out-format sets the output sample format (default FLOAT64_LE); --dither enables HP-TPDF dither
on both outputs (an integer --out-format is needed; sample rate 48000); --delay gives both
outputs a maxdelay of 48 000 frames and new delays (seeded, up to 48 000) every 300 periods;
--subdelay gives both inputs and both outputs a sub-sample delay filter (sdf_length 31) and new
values (seeded, in (-100, 100)) every 300 periods."""
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
    rng = np.random.default_rng(5)
    for o in range(2):
        for i in range(2):
            h = rng.standard_normal(1048576) * np.exp(-np.arange(1048576) / 2e5) / 2000.0
            nu.add_filter(i, o, h)
    nu.finalize()
    x = rng.standard_normal((8, L0, 2)) * 0.1
    import gc
    gc.disable()                       # the timed loop allocates one small array per period
    ts = []
    drng = np.random.default_rng(9)
    n_changes = n_sd_changes = 0
    for s in range(steps + 256):
        if a.delay and s % 300 == 299:
            for o in range(2):
                nu.set_delay(bf.OUT, o, int(drng.integers(0, 48001)))
            n_changes += 1
        if a.subdelay and s % 300 == 299:
            for io in (bf.IN, bf.OUT):
                for c in range(2):
                    nu.set_subdelay(io, c, int(drng.integers(-99, 100)))
            n_sd_changes += 1
        t0 = time.perf_counter()
        st, _ = nu.block(x[s & 7])
        ts.append(time.perf_counter() - t0)
        assert st == 0
    ts = np.array(ts[256:]) * 1e3
    # the periods in which every segment has a block to launch (the schedule's worst case), as
    # opposed to the rare host-side hiccups that land anywhere
    ratio = seg_len[-1] // L0
    full = ts[[i for i in range(len(ts)) if (i + 256 + 1) % ratio == 0]]
    print(json.dumps({
        "workload": "configs[4]: 2-in/2-out, %d taps, float64, partitions %s x %s" % (nu.taps, seg_len, seg_blk),
        "out_format": a.out_format, "dithered_outputs": [0, 1] if a.dither else [],
        "delayed_outputs": {"maxdelay": 48000, "changes_every_periods": 300, "changes": n_changes} if a.delay else None,
        "subdelay": {"sdf_length": 31, "inputs": [0, 1], "outputs": [0, 1], "changes_every_periods": 300,
                     "changes": n_sd_changes} if a.subdelay else None,
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
