"""sha256 of the output blocks of a fixed list of block-pass cases, from seeded numpy inputs.

    python tools/pass_bits.py [--out FILE] [case ...]

One JSON object {case: {"sha256": ..., "nonzero": true, "path": [block_mode, uses_wave_fft, pair launches,
graph replays]}}.  Run on the commit before the kernel launches moved out of csrc/bfhip.hip (851e57b) and
committed as tests/golden/pass_bits_parent.json, it pins what tools/mac_bits.py, plan_bits.py and
channel_bits.py do not: which transform path (LDS FFT, wave FFT, the global-memory FFT above 8192) feeds
which schedule and entry point -- a ring slot, a twiddle table, a chunk count or a stream taken from the
wrong place changes bits below any tolerance.  tests/test_gpu_pass_bits.py asserts the same values on the
tree it runs in.

Every case is 2 inputs x 2 outputs, N = 2, seeded IRs of N L taps, S24_4LE in, FLOAT_LE out, N + 3 blocks,
f32, unless it says otherwise.  L is the smallest its path accepts: LDS 256, wave 1024 (BFHIP_FFT_WAVE=1),
big 16384.  Outputs are hashed in block order, after flush and sync.

Twins.  The schedules of one transform path are meant to give the same bits (block_owed's and
block_pair_dev's comments say so).  On the parent, per path, block_dev in order, the phase calls, the fused
outputs_inputs call, the pipelined / deferred / ping-pong schedules and real-time mode with graph replay all
hash equal, and so do block pairs and the same blocks run singly, the four-chunk plan in order and deferred;
case_list() marks them (`twin`) and the test asserts the equality beside the golden value.  The f64, level
and coefficient cases have no twin.

The level-kernel cases (a cascade, an N-way input mix, a one-block cross-fade in one plan) run on wave and
on big: plan_bits' `big` case is a plain crossbar and holds none of the three.  The four-chunk case is
plan_bits' split_along_p (1 x 1, N = 16, BFHIP_MAC_DIAG=0) at L = 1024, where the crossbar kernel has two
tiles: BFHIP_MAC_TARGET_WGS=8 gives the four chunks.  The pair cases are 2 x 8: an entry is dense only with
all 8 outputs of its group.
"""
import contextlib
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import plan_bits  # noqa: E402
from mac_bits import _ir  # noqa: E402

PATHS = {"lds": (256, {}), "wave": (1024, {"BFHIP_FFT_WAVE": 1}), "big": (16384, {})}
ENV_KEYS = plan_bits.EXTRA_ENV_KEYS + ("BFHIP_LONG_WINDOW", "BFHIP_LOOKAHEAD", "BFHIP_MAC_TARGET_WGS", "BFHIP_OVERLAP",
                                       "BFHIP_MAC_DIAG", "BFHIP_FFT_WAVE", "BFHIP_DEFER")
SEQUENTIAL, PIPELINED, DEFERRED, PINGPONG = 0, 1, 2, 3


@contextlib.contextmanager
def env_set(**kv):
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    assert set(kv) <= set(ENV_KEYS), kv
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---------------------------------------------------------------- engines

def xbar(L, N=2, I=2, O=2, rs=4, in_order=True, pairs=False, dev_set=False):
    """plan_bits' crossbar; in_order: set_overlap(0), else the environment chooses the schedule; dev_set: set 0
    comes from device taps (add_coeff_dev) -> (engine, sets)"""
    e = plan_bits._engine(N, I, O, rs, "FLOAT_LE" if rs == 4 else "FLOAT64_LE", length=L)
    if in_order:
        e.set_overlap(0)
    if pairs:
        e.enable_pairs(True)
    if dev_set:
        import torch
        taps = torch.from_numpy(np.ascontiguousarray(_ir(4321, L * N, I), e.dt)).to("cuda")
        torch.cuda.synchronize()
        first = e.add_coeff_dev(taps, L * N)
        sets = [first] + plan_bits._xbar(e, N, I, O, length=L)
        e.finalize()
        e.set_coeff(0, first)          # filter 0 was given the host copy of the same taps: the device-made set instead
        return e, sets
    sets = plan_bits._xbar(e, N, I, O, length=L)
    e.finalize()
    return e, sets


def levels(L):
    """plan_bits' cascade_mix at length L, its sink cross-fading -> (engine, [the set it fades to])"""
    N = 2
    e = plan_bits._engine(N, 2, 2, length=L)
    e.set_overlap(0)
    c = [e.add_coeff(_ir(100 + k, L * N, 2)) for k in range(4)]
    f0 = e.add_filter(in_ch=[0], out_ch=[0], coeff=c[0])               # a cascade source that feeds an output too
    f1 = e.add_filter(in_ch=[1], coeff=c[1])
    e.add_filter(in_ch=[0], in_scale=[0.25], in_f=[f0, f1], in_fscale=[0.5, -1.25], out_ch=[1], out_scale=[0.8],
                 coeff=c[2], crossfade=True)
    e.finalize()
    return e, [c[3]]


# ---------------------------------------------------------------- runners: (engine, sets, blocks) -> [bytes per block]

def _dev_buffers(e, blocks):
    import torch
    srcs = [torch.from_numpy(b).to("cuda") for b in blocks]
    outs = [torch.zeros(e.out_bytes, dtype=torch.uint8, device="cuda") for _ in blocks]
    torch.cuda.synchronize()                     # the engine's streams do not order with torch's
    return torch, srcs, outs


def _collect(e, outs):
    e.flush()
    assert e.sync() == 0
    return [o.cpu().numpy().tobytes() for o in outs]


def run_block_dev(e, sets, blocks):
    _, srcs, outs = _dev_buffers(e, blocks)
    for s, o in zip(srcs, outs):
        e.block_dev(s, o)
    return _collect(e, outs)


def _spectra(torch, e, n):
    z = [torch.zeros(e.n_out, e.L, 2, dtype=torch.float32 if e.rs == 4 else torch.float64, device="cuda")
         for _ in range(n)]
    torch.cuda.synchronize()
    return z


def run_phases(e, sets, blocks):
    torch, srcs, outs = _dev_buffers(e, blocks)
    z = _spectra(torch, e, 1)[0]
    for s, o in zip(srcs, outs):
        e.inputs_dev(s)
        e.mac_dev(z)
        e.outputs_dev(z, 0, e.n_out, o)
        e.advance()
    return _collect(e, outs)


def run_fused(e, sets, blocks):
    """the outputs of block k - 2 with the inputs of block k (bench.py's pipeline over several devices)"""
    torch, srcs, outs = _dev_buffers(e, blocks)
    z = _spectra(torch, e, 3)
    n = len(blocks)
    for k in range(n):
        if k >= 2:
            e.outputs_inputs_dev(z[(k - 2) % 3], 0, e.n_out, outs[k - 2], srcs[k])
        else:
            e.inputs_dev(srcs[k])
        e.mac_dev(z[k % 3])
        e.advance()
    for k in (n - 2, n - 1):
        e.outputs_dev(z[k % 3], 0, e.n_out, outs[k])
    return _collect(e, outs)


def run_pairs(e, sets, blocks):
    _, srcs, outs = _dev_buffers(e, blocks)
    for k in range(1, len(blocks), 2):
        e.block_pair_dev(srcs[k - 1], outs[k - 1], srcs[k], outs[k])
    if len(blocks) % 2:
        e.block_dev(srcs[-1], outs[-1])
    return _collect(e, outs)


def run_rt(e, sets, blocks):
    e.rt_begin(0)
    got = []
    for b in blocks:
        st, raw = e.rt_block(b)
        assert st == 0, st
        got.append(raw.tobytes())
    e.graph_replays = e.rt_stats()["graph"]
    e.rt_end()
    return got


def run_host(e, sets, blocks, actions=None):
    got = []
    for k, b in enumerate(blocks):
        if actions and k in actions:
            actions[k](e, sets)
        st, raw = e.block(b)
        assert st == 0, (k, st)
        got.append(raw.tobytes())
    return got


def run_fade(e, sets, blocks):
    return run_host(e, sets, blocks, {3: lambda e, x: e.set_coeff(2, x[0])})


def run_coeff(e, sets, blocks):
    """set 0 was made on the device; partition 1 of it is replaced by that of set 3, in the reference's layout;
    then the whole set is read back in that layout (the first item hashed) and the blocks run"""
    donor = e.read_coeff_processed(sets[3], e.N)
    e.refresh_coeff_processed(sets[0], 1, np.ascontiguousarray(donor[1]))
    back = e.read_coeff_processed(sets[0], e.N)
    assert np.array_equal(back[1], donor[1]) and not np.array_equal(back[0], donor[0])
    return [back.tobytes()] + run_host(e, sets, blocks)


# ---------------------------------------------------------------- cases

def case_list():
    """name -> dict(env, L, make=() -> (engine, sets), run, I, blocks, seed, want={index into path: value or
    ">0"}, twin=name of the case whose hash this one's equals)"""
    cs = {}

    def add(name, path, make, run, env=None, want=None, twin=None, I=2, blocks=5, seed=41):
        L, penv = PATHS[path]
        want = dict(want or {})
        want.setdefault(1, path == "wave")
        cs[name] = dict(env=dict({"BFHIP_LONG_WINDOW": 0}, **penv, **(env or {})), L=L, make=lambda: make(L), run=run,
                        I=I, blocks=blocks, seed=seed, want=want, twin=twin)

    for p in PATHS:
        first = "block_dev_" + p
        add(first, p, xbar, run_block_dev, want={0: SEQUENTIAL})
        add("block_dev_f64_" + p, p, lambda L: xbar(L, rs=8), run_block_dev, want={0: SEQUENTIAL})
        add("phases_" + p, p, xbar, run_phases, twin=first)
        add("fused_" + p, p, xbar, run_fused, twin=first)
    add("pipelined_lds", "lds", lambda L: xbar(L, in_order=False), run_block_dev, env={"BFHIP_OVERLAP": 1},
        want={0: PIPELINED}, twin="block_dev_lds")
    add("deferred_wave", "wave", lambda L: xbar(L, in_order=False), run_block_dev,
        env={"BFHIP_DEFER": 1, "BFHIP_OVERLAP": 0}, want={0: DEFERRED}, twin="block_dev_wave")
    add("pingpong_wave", "wave", lambda L: xbar(L, in_order=False), run_block_dev, env={"BFHIP_OVERLAP": 1},
        want={0: PINGPONG}, twin="block_dev_wave")
    # split_along_p of plan_bits on the wave path: the in-place sum of do_outputs, and that of block_owed
    four = {"BFHIP_MAC_DIAG": 0, "BFHIP_MAC_TARGET_WGS": 8}
    add("chunks4_in_order_wave", "wave", lambda L: xbar(L, 16, 1, 1), run_block_dev, env=four, want={0: SEQUENTIAL},
        I=1, blocks=19, seed=42)
    add("chunks4_deferred_wave", "wave", lambda L: xbar(L, 16, 1, 1, in_order=False), run_block_dev,
        env=dict(four, BFHIP_DEFER=1, BFHIP_OVERLAP=0), want={0: DEFERRED}, twin="chunks4_in_order_wave", I=1,
        blocks=19, seed=42)
    for p in ("lds", "wave"):
        add("single_2x8_" + p, p, lambda L: xbar(L, O=8), run_block_dev, want={0: SEQUENTIAL, 2: 0}, seed=43)
        add("pairs_2x8_" + p, p, lambda L: xbar(L, O=8, pairs=True), run_pairs, want={2: ">0"}, twin="single_2x8_" + p,
            seed=43)
        add("rt_graph_" + p, p, xbar, run_rt, want={3: ">0"}, twin="block_dev_" + p)
    for p in ("wave", "big"):
        add("levels_" + p, p, levels, run_fade, blocks=6, seed=44)
    for p in ("lds", "big"):
        add("coeff_" + p, p, lambda L: xbar(L, dev_set=True), run_coeff, seed=45)
    return cs


def run_case(c):
    """-> {"sha256", "nonzero", "path"}"""
    import cases
    import torch
    assert torch.cuda.is_available()     # torch's own HIP runtime has to start before libbfhip.so loads the system's
    with env_set(**c["env"]):
        blocks = cases.raw_blocks(c["seed"], c["blocks"], c["L"], c["I"], "S24_4LE")
        e, sets = c["make"]()
        e.graph_replays = 0
        try:
            got = c["run"](e, sets, blocks)
            e.sync()
            path = [int(e.block_mode), bool(e.uses_wave_fft), int(e.pair_launches), int(e.graph_replays)]
        finally:
            e.close()
    h = hashlib.sha256()
    for g in got:
        h.update(g)
    return {"sha256": h.hexdigest(), "nonzero": all(any(g) for g in got[-2:]), "path": path}


def shows_its_branch(c, got):
    return all(got["path"][i] > 0 if v == ">0" else got["path"][i] == v for i, v in c["want"].items())


def main(argv):
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    cs = case_list()
    names = argv or list(cs)
    res = {}
    for n in names:
        res[n] = run_case(cs[n])
        assert res[n]["nonzero"] and shows_its_branch(cs[n], res[n]), (n, res[n])
        print(n, res[n]["sha256"], res[n]["path"], file=sys.stderr, flush=True)
    for n in names:
        t = cs[n]["twin"]
        if t in res:
            print("twin", n, t, res[n]["sha256"] == res[t]["sha256"], file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1, sort_keys=True) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
