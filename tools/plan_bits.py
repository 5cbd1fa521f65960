"""sha256 of the output blocks of a fixed list of plan-builder cases, from seeded numpy inputs.

    python tools/plan_bits.py [--out FILE] [case ...]

One JSON object {case: {"sha256": ..., "nonzero": true, "path": [block_mode, uses_diag_mac,
uses_stream_layout, window_blocks], "bytes": [block, mac]}}.  Run on the commit before a change of the
plan builder (csrc/plan.hip) and committed as tests/golden/plan_bits_parent.json, it pins what a reshuffle
of the builder can alter without failing a tolerance test: the order an output's terms are summed in, the
chunk split, the kernel an entry is given.  tests/test_gpu_plan_bits.py asserts the same values on the
tree it runs in.  (The long-window, look-ahead and far-tier layouts are pinned by tools/mac_bits.py and
tests/test_gpu_lookahead_far.py.)

Every case is f32, L = 512, N = 3 or 4, S24_4LE in, FLOAT_LE out, seeded IRs of L N taps, N + 3 blocks,
unless it says otherwise; path and bytes are read after the last block, from the plan built last.
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

import mac_bits  # noqa: E402
from mac_bits import _ir  # noqa: E402

L = 512
EXTRA_ENV_KEYS = ("BFHIP_COEFF_STREAM", "BFHIP_DIAG_SPLIT", "BFHIP_MAC_NT", "BFHIP_MAC_UNROLL", "BFHIP_LONG_CHUNKS",
                  "BFHIP_LOOKAHEAD_FAR")


@contextlib.contextmanager
def env_set(**kv):
    """mac_bits.env_set for its keys, the same for the other knobs the plan builder reads"""
    old = {k: os.environ.pop(k, None) for k in EXTRA_ENV_KEYS}
    try:
        with mac_bits.env_set(**kv):
            yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _engine(N, I, O, rs=4, outfmt="FLOAT_LE", length=L):
    import brutefir_amd as bf
    e = bf.Engine(length, N, rs, I, O)
    e.set_interleaved(0, "S24_4LE")
    e.set_interleaved(1, outfmt)
    return e


def _xbar(e, N, I, O, crossfade=False, length=L):
    """I x O crossbar on outputs 0 .. O-1: filter o I + i takes input i to output o -> its coefficient sets"""
    sets = []
    for o in range(O):
        for i in range(I):
            sets.append(e.add_coeff(_ir(4321 + o * I + i, length * N, I)))
            e.add_filter(in_ch=[i], out_ch=[o], coeff=sets[-1], crossfade=crossfade)
    return sets


def cascade_mix():
    N = 3
    e = _engine(N, 2, 2)
    c = [e.add_coeff(_ir(100 + k, L * N, 2)) for k in range(3)]
    f0 = e.add_filter(in_ch=[0], out_ch=[0], coeff=c[0])               # a cascade source that feeds an output too
    f1 = e.add_filter(in_ch=[1], coeff=c[1])
    e.add_filter(in_ch=[0], in_scale=[0.25], in_f=[f0, f1], in_fscale=[0.5, -1.25], out_ch=[1], out_scale=[0.8],
                 coeff=c[2])
    e.finalize()
    return e, []


def fade_and_dirac():
    N = 4
    e = _engine(N, 2, 2)
    for o in range(2):
        for i in range(2):
            c = -1 if (o, i) == (1, 1) else e.add_coeff(_ir(200 + o * 2 + i, L * N, 2))
            e.add_filter(in_ch=[i], out_ch=[o], coeff=c, crossfade=True)
    extra = [e.add_coeff(_ir(210, L * N, 2))]
    e.finalize()
    return e, extra


def twice_from_one_ring():
    N = 3
    e = _engine(N, 2, 2)
    c = [e.add_coeff(_ir(300 + k, L * N, 2)) for k in range(4)]
    e.add_filter(in_ch=[0], out_ch=[0], coeff=c[0])
    e.add_filter(in_ch=[0], out_ch=[0], coeff=c[1])                    # the same (ring, delay) key again
    e.add_filter(in_ch=[0], out_ch=[0], coeff=c[2], delayblocks=1)
    e.add_filter(in_ch=[1], out_ch=[1, 0], out_scale=[1.0, -0.5], coeff=c[3])
    for f in range(4):
        e.set_filter_name(f, 3 - f)
    e.finalize()
    return e, []


def runtime_changes():
    N = 4
    e = _engine(N, 3, 3)
    _xbar(e, N, 3, 3)
    extra = [e.add_coeff(_ir(410, L * N, 3))]
    e.finalize()
    return e, extra


def powersave():
    N = 3
    e = _engine(N, 2, 2)
    e.set_powersave(0.5)
    _xbar(e, N, 2, 2)
    e.finalize()
    return e, []


def split_along_p():
    N = 16
    e = _engine(N, 1, 1)
    _xbar(e, N, 1, 1)
    e.finalize()
    return e, []


def subset_and_single(rs=4, outfmt="FLOAT_LE", rest=True):
    """inputs 0 .. 2 to outputs 0 .. 2 (three terms of eight: the subset path); with `rest`, input 3 alone to
    output 3 with fewer partitions (the single-term path) and a short filter from input 0 to output 4, which
    makes the entry of input 0 one of unequal lengths (the generic path)"""
    N = 4
    e = _engine(N, 4 if rest else 3, 5 if rest else 3, rs, outfmt)
    _xbar(e, N, 3, 3)
    if rest:
        e.add_filter(in_ch=[3], out_ch=[3], coeff=e.add_coeff(_ir(510, L * 2, 3)))
        e.add_filter(in_ch=[0], out_ch=[4], coeff=e.add_coeff(_ir(511, L * 3, 3)))
    e.finalize()
    return e, []


def diag(lengths):
    def make():
        N = 8
        e = _engine(N, len(lengths), len(lengths))
        for c, n in enumerate(lengths):
            e.add_filter(in_ch=[c], out_ch=[c], coeff=e.add_coeff(_ir(700 + c, L * n, 1)))
        e.finalize()
        return e, []
    return make


def shard(half):
    """3 inputs, 8 outputs (one group), 10 filters: input 0 to every output (the whole plan's dense entry), input
    1 to output 5 and input 2 to output 1.  Half a owns outputs 0 .. 3, half b outputs 4 .. 7: the dense entry
    keeps four of its eight terms (a subset entry) and the entry of the other half's single filter loses all of
    its terms.  Eight outputs, not the four of a 4 x 4 network: an entry is dense only with all OG = 8 terms."""
    def make():
        N = 3
        e = _engine(N, 3, 8)
        outs = [(0, o) for o in range(8)] + [(1, 5), (2, 1)]
        for k, (i, o) in enumerate(outs):
            f = e.add_filter(in_ch=[i], out_ch=[o], coeff=e.add_coeff(_ir(800 + k, L * N, 3)))
            e.set_filter_active(f, int((o < 4) == (half == "a")))
        for o in range(8):
            e.set_output_active(o, int((o < 4) == (half == "a")))
        e.finalize()
        return e, []
    return make


def stream_layout():
    N = 3
    e = _engine(N, 8, 8)
    _xbar(e, N, 8, 8)
    extra = [e.add_coeff(_ir(910, L * N, 8))]
    e.finalize()
    return e, extra


def big():
    N, LB = 2, 16384
    e = _engine(N, 2, 2, length=LB)
    _xbar(e, N, 2, 2, length=LB)
    e.finalize()
    return e, []


def _new_block(seed):
    return _ir(seed, L, 1)


def case_list():
    """name -> dict(env, make=() -> (engine, extra sets), I, L, blocks, seed, actions={block: f(engine, extra)},
    zero_in=[input channels of silence], amplitude, want={index into path: value the case is there for})"""
    std = {"BFHIP_LONG_WINDOW": 0}
    cs = {}
    cs["cascade_mix"] = dict(env=std, make=cascade_mix, I=2, blocks=6, seed=21)
    cs["fade_and_dirac"] = dict(
        env=std, make=fade_and_dirac, I=2, blocks=7, seed=22,
        actions={3: lambda e, x: e.set_coeff(3, x[0]),                 # from the dirac: prevcoeff = -1
                 4: lambda e, x: e.set_coeff(0, -1)})                  # to the dirac
    cs["twice_from_one_ring"] = dict(env=std, make=twice_from_one_ring, I=2, blocks=6, seed=23)
    cs["runtime_changes"] = dict(
        env=std, make=runtime_changes, I=3, blocks=7, seed=24,
        actions={1: lambda e, x: e.set_delayblocks(2, 1),
                 2: lambda e, x: (e.set_scale(4, 0, 0, 0.5), e.set_scale(5, 1, 0, -0.75)),
                 3: lambda e, x: e.set_coeff(7, x[0]),
                 5: lambda e, x: e.update_coeff_block(0, 1, _new_block(420))})
    # (input at 0.3 of full scale: a window of the usual 0.1 peaks below the floor of 0.5 and all would be silence)
    cs["powersave"] = dict(env=std, make=powersave, I=2, blocks=6, seed=25, zero_in=[1], amplitude=0.3)
    # one entry: the cost model keeps S = 1 and a one-to-one plan takes the diag kernel; held to the crossbar
    # kernel and to S = 4 > 2 by the two knobs, the entry is split along p into four parts
    cs["split_along_p"] = dict(env=dict(std, BFHIP_MAC_DIAG=0, BFHIP_MAC_TARGET_WGS=4), make=split_along_p, I=1,
                               blocks=19, seed=26, want={1: False})
    cs["subset_and_single"] = dict(env=std, make=subset_and_single, I=4, blocks=7, seed=27)
    cs["subset_f64"] = dict(env=std, make=lambda: subset_and_single(8, "FLOAT64_LE", rest=False), I=3, blocks=7,
                            seed=27)
    cs["diag_parts"] = dict(env=std, make=diag([8, 8, 8, 8]), I=4, blocks=11, seed=28, want={1: True})
    cs["diag_unequal"] = dict(env=std, make=diag([8, 8, 3, 1]), I=4, blocks=11, seed=29)
    cs["shard_a"] = dict(env=std, make=shard("a"), I=3, blocks=6, seed=30)
    cs["shard_b"] = dict(env=std, make=shard("b"), I=3, blocks=6, seed=30)
    cs["stream_layout"] = dict(
        env=dict(std, BFHIP_COEFF_STREAM=2, BFHIP_MAC_TARGET_WGS=8), make=stream_layout, I=8, blocks=6, seed=31,
        actions={2: lambda e, x: e.update_coeff_block(9, 1, _new_block(920)),
                 4: lambda e, x: e.set_coeff(20, x[0])}, want={2: True})
    cs["big"] = dict(env=std, make=big, I=2, L=16384, blocks=5, seed=32, want={1: False})
    for c in cs.values():
        c.setdefault("L", L)
    return cs


def run_case(c):
    """-> {"sha256", "nonzero", "path", "bytes"}"""
    import cases
    with env_set(**c["env"]):
        blocks = cases.raw_blocks(c["seed"], c["blocks"], c["L"], c["I"], "S24_4LE", c.get("amplitude", 0.1))
        for ch in c.get("zero_in", []):
            for b in blocks:
                b[:, ch] = 0
        return _run(c, blocks)


def _run(c, blocks):
    e, extra = c["make"]()
    h = hashlib.sha256()
    nonzero = False
    try:
        for k, b in enumerate(blocks):
            if k in c.get("actions", {}):
                c["actions"][k](e, extra)
            st, raw = e.block(b)
            assert st == 0, (k, st)
            out = raw.tobytes()
            nonzero = nonzero or any(out)
            h.update(out)
        e.sync()
        path = [int(e.block_mode), bool(e.uses_diag_mac), bool(e.uses_stream_layout), int(e.window_blocks)]
        ab = e.algorithmic_bytes()
    finally:
        e.close()
    return {"sha256": h.hexdigest(), "nonzero": bool(nonzero), "path": path, "bytes": [ab["block"], ab["mac"]]}


def shows_its_branch(c, got):
    return all(got["path"][i] == v for i, v in c.get("want", {}).items())


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
        print(n, res[n]["sha256"], res[n]["path"], res[n]["bytes"], file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1, sort_keys=True) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
