"""sha256 of the output blocks of a fixed list of channel-stage cases, from seeded numpy inputs.

    python tools/channel_bits.py [--out FILE] [--oracle] [case ...]

One JSON object {case: {"sha256": ..., "sha256_off": ..., "nonzero": true, "path": [block_mode,
uses_wave_fft, output_lag, real-time blocks replayed from a graph]}}.  Run on the commit before a change of
the channel stage (csrc/channels.hip: N:1 virtual-to-physical channels, integer delay lines and mutes,
sub-sample delay filters, the dither pass and its late variant, the planar copies of wide sides) and
committed as tests/golden/channel_bits_parent.json, it pins what a move of that code can alter without
failing a tolerance test: the order a shared output's members are mixed in, the slot a delay line is in
after a change, where a dither chain's table walk starts, what an unowned byte holds.
tests/test_gpu_channel_bits.py asserts the same values on the tree it runs in.

sha256 covers the raw output bytes of every block, then every virtual output's overflow record after the
last block.  sha256_off is the same case with the channel stage neutralised: identity maps (a physical
input that several virtual ones shared is handed over once per virtual channel), delays 0, no mutes, no
sub-sample filters, no dither, BFHIP_WIDE_IO=0.  A case shows its branch when the two differ -- except
where the case says `transparent`: the planar copies of a wide side move bytes and change none, so there
the two hashes must be EQUAL and the path (deferred output, the schedule whose fused launch the transposes
surround) is what shows the branch.

Every case is f32, L = 256, N = 2, S24_4LE in, FLOAT_LE out, 10 blocks (a delay of 2L + 3 has then wrapped
its ring of full fragments), every virtual input to every virtual output through a seeded IR of L N taps,
unless it says otherwise.  --oracle runs the cases the oracle can express (no shards, no real-time mode)
through oracle/bforacle.py on the CPU and checks the same well-formedness: status 0, sound, twin differs.
"""
import contextlib
import copy
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

L = 256
ENV_KEYS = ("BFHIP_WIDE_IO", "BFHIP_FFT_WAVE", "BFHIP_OVERLAP", "BFHIP_DEFER", "BFHIP_LONG_WINDOW", "BFHIP_MAC_DIAG")
SAMPLE_BYTES = {"S16_LE": 2, "S24_4LE": 4, "S32_LE": 4, "FLOAT_LE": 4, "FLOAT64_LE": 8}
MODE_DEFERRED = 2
PATTERN = 0xA5                         # what a shard's caller left in the shared output buffer


@contextlib.contextmanager
def env_set(**kv):
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    try:
        os.environ.update({k: str(v) for k, v in kv.items()})
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def case(**kw):
    """the defaults of a case; delay / maxdelay / subdelay: {(io, virtual channel): value}, dither: PHYSICAL
    outputs, actions: {block: [("delay" | "mute" | "subdelay", io, virtual channel, value)]}, own: the virtual
    outputs a shard engine owns (None: all), hash_owned: hash the owned bytes only"""
    c = dict(L=L, N=2, rs=4, n_in=2, n_out=2, in_map=None, out_map=None, in_fmt="S24_4LE", out_fmt="FLOAT_LE",
             blocks=10, amplitude=0.1, gain={}, delay={}, maxdelay={}, sdf=0, subdelay={}, dither=(), rate=200,
             actions={}, own=None, hash_owned=False, rt=False, env={}, transparent=False, want_mode=None)
    c.update(kw)
    for io, key, n in ((0, "in_map", c["n_in"]), (1, "out_map", c["n_out"])):
        if c[key] is None:
            c[key] = list(range(n))
    return c


N_TO_1_IN = dict(n_in=3, in_map=[0, 1, 0], delay={(0, 0): 5, (0, 1): 0, (0, 2): 2 * L + 3},
                 maxdelay={(0, 0): 3 * L, (0, 2): 3 * L})


def case_list():
    cs = {}
    # the long line shrinks to the short buffers and grows back; the other member is muted for two blocks (its line
    # must not advance meanwhile)
    cs["n_to_1_in"] = case(seed=41, **N_TO_1_IN,
                           actions={3: [("mute", 0, 0, 1)], 4: [("delay", 0, 2, L - 7)], 5: [("mute", 0, 0, 0)],
                                    7: [("delay", 0, 2, 2 * L + 3)]})
    cs["n_to_1_out"] = case(seed=42, n_out=4, out_map=[0, 1, 0, 1], out_fmt="S16_LE", amplitude=0.3,
                            gain={1: 10.0, 3: 10.0},
                            delay={(1, 0): 0, (1, 1): 5, (1, 2): 2 * L + 3, (1, 3): L},
                            maxdelay={(1, v): 3 * L for v in range(4)},
                            actions={3: [("mute", 1, 2, 1)], 5: [("mute", 1, 2, 0)]})
    # virtual 1: 1:1 and filtered, read from raw; virtual 0: a filtered member of physical 0, whose other member
    # (2) gets the integer part; 3: 1:1 and unfiltered (its integer part is the sound card interface's business)
    cs["subdelay_in"] = case(seed=43, n_in=4, in_map=[0, 1, 0, 2], sdf=15, subdelay={(0, 0): -20, (0, 1): 37},
                             delay={(0, 2): 3}, maxdelay={(0, 2): L},
                             actions={5: [("subdelay", 0, 1, 12)]})
    # virtual 0: 1:1 and filtered, a group of one: the delay and the mute set on it are not the engine's to apply
    cs["subdelay_out"] = case(seed=44, n_out=4, out_map=[0, 1, 1, 2], sdf=15, subdelay={(1, 0): 37, (1, 1): -45},
                              delay={(1, 0): 7, (1, 2): 3}, maxdelay={(1, 0): L, (1, 2): L},
                              actions={0: [("mute", 1, 0, 1)]})
    # physical 0: 1:1, dithered in K3's pass; 1: shared, 2: sub-sample filtered -- both dithered late
    dith = dict(n_out=5, out_map=[0, 1, 1, 2, 3], out_fmt="S16_LE", sdf=15, subdelay={(1, 3): 25}, dither=(0, 1, 2),
                delay={(1, 2): 5}, maxdelay={(1, 2): L}, amplitude=0.3, gain={1: 12.0, 2: 12.0})
    cs["dither_early_late"] = case(seed=45, **dith)
    # maxdelay -1 beside a sub-sample filter stays a fixed delay (input 2); a delay above a positive
    # limit starts at the limit (output 0)
    cs["maxdelay_fixed"] = case(seed=46, n_in=3, in_map=[0, 1, 0], n_out=3, out_map=[0, 0, 1], sdf=15,
                                subdelay={(0, 0): 10}, delay={(0, 2): 7, (1, 0): 300, (1, 1): 2},
                                maxdelay={(0, 2): -1, (1, 0): 100, (1, 1): L})
    # one configuration, two engines: the owner has the shared pair (1, 2) and the filtered output 3, both
    # dithered late; the other engine owns outputs 0 and 4 and so has no time-sample buffer
    shard = dict(n_out=5, out_map=[0, 1, 1, 2, 3], out_fmt="S16_LE", sdf=15, subdelay={(1, 3): 25}, dither=(1, 2),
                 delay={(1, 2): 5}, maxdelay={(1, 2): L}, amplitude=0.3, gain={1: 12.0, 2: 12.0})
    cs["shard_owner"] = case(seed=47, own=[1, 2, 3], hash_owned=True, **shard)
    cs["shard_foreign"] = case(seed=47, own=[0, 4], **shard)
    wide = dict(L=1024, n_in=4, n_out=4, in_fmt="S32_LE", out_fmt="S32_LE", transparent=True, want_mode=MODE_DEFERRED,
                env=dict(BFHIP_WIDE_IO=1, BFHIP_FFT_WAVE=1, BFHIP_OVERLAP=0))
    cs["wide_deferred"] = case(seed=48, **wide)
    cs["wide_deferred_shard"] = case(seed=48, own=[0, 3], **wide)
    cs["big_shared_out"] = case(seed=49, L=16384, N=1, n_in=1, n_out=2, out_map=[0, 0], delay={(1, 1): 5},
                                maxdelay={(1, 1): 16384})
    cs["rt_n_to_1"] = case(seed=41, rt=True, blocks=6, **N_TO_1_IN,
                           actions={1: [("mute", 0, 0, 1)], 2: [("delay", 0, 2, L - 7)], 3: [("mute", 0, 0, 0)],
                                    4: [("delay", 0, 2, 2 * L + 3)]})
    f64 = dict(dith, subdelay={(1, 1): -45, (1, 3): 25})
    cs["f64_mix"] = case(seed=50, rs=8, **f64)
    return cs


def neutral(c):
    """the feature-off twin"""
    o = copy.deepcopy(c)
    o.update(in_map=list(range(c["n_in"])), out_map=list(range(c["n_out"])), delay={}, maxdelay={}, sdf=0, subdelay={},
             dither=(), actions={}, env=dict(c["env"], BFHIP_WIDE_IO=0) if "BFHIP_WIDE_IO" in c["env"] else c["env"])
    return o


def oracle_can(c):
    return c["own"] is None and not c["rt"]


def _ir(seed, taps, n_in):
    import cases
    return cases.make_ir(np.random.default_rng(seed), taps, n_in)


def make_engine(c, engine_cls):
    e = engine_cls(c["L"], c["N"], c["rs"], c["n_in"], c["n_out"])
    for io, m, fmt in ((0, c["in_map"], c["in_fmt"]), (1, c["out_map"], c["out_fmt"])):
        if m != list(range(len(m))):
            e.map_channels(io, m)
        e.set_interleaved_phys(io, fmt, max(m) + 1)
    if c["sdf"]:
        e.enable_subdelay(c["sdf"])
        for (io, v), value in sorted(c["subdelay"].items()):
            e.set_subdelay(io, v, value)
    for (io, v), d in sorted(c["delay"].items()):
        e.set_delay(io, v, d)
    for (io, v), d in sorted(c["maxdelay"].items()):
        e.set_maxdelay(io, v, d)
    if c["dither"]:
        e.enable_dither(list(c["dither"]), c["rate"])
    for o in range(c["n_out"]):
        for i in range(c["n_in"]):
            f = e.add_filter(in_ch=[i], out_ch=[o], out_scale=[c["gain"].get(o, 1.0)],
                             coeff=e.add_coeff(_ir(1000 * c["seed"] + o * c["n_in"] + i, c["L"] * c["N"], c["n_in"])))
            if c["own"] is not None:
                e.set_filter_active(f, int(o in c["own"]))
    if c["own"] is not None:
        for o in range(c["n_out"]):
            e.set_output_active(o, int(o in c["own"]))
    if hasattr(e, "finalize"):
        e.finalize()
    return e


def inputs(c, on):
    """the raw blocks of a case: seeded per PHYSICAL input of the case as listed (`on`); the twin's identity map
    gets the column of that physical input once per virtual channel"""
    import cases
    blocks = cases.raw_blocks(c["seed"], c["blocks"], c["L"], max(on["in_map"]) + 1, c["in_fmt"], c["amplitude"])
    if c["in_map"] != on["in_map"]:
        blocks = [np.ascontiguousarray(b[:, on["in_map"]]) for b in blocks]
    return blocks


def owned_bytes(c, out):
    ss = SAMPLE_BYTES[c["out_fmt"]]
    n_phys = max(c["out_map"]) + 1
    phys = sorted({c["out_map"][v] for v in c["own"]})
    return out[:c["L"] * n_phys * ss].reshape(c["L"], n_phys, ss)[:, phys, :].tobytes()


def act(e, a):
    {"delay": e.set_delay, "mute": e.set_mute, "subdelay": e.set_subdelay}[a[0]](a[1], a[2], a[3])


def run_one(c, on, engine_cls):
    """-> (sha256, nonzero, path)"""
    with env_set(BFHIP_LONG_WINDOW=0, **c["env"]):
        e = make_engine(c, engine_cls)
        h = hashlib.sha256()
        nonzero = False
        native = hasattr(e, "close")
        try:
            if c["rt"]:
                e.rt_begin(0)
            for k, b in enumerate(inputs(c, on)):
                for a in c["actions"].get(k, []):
                    act(e, a)
                if not native:
                    st, raw = e.block(b)
                else:
                    out = np.full(e.out_bytes, PATTERN if c["own"] is not None else 0, np.uint8)
                    st, raw = e.rt_block(b, out=out) if c["rt"] else e.block(b, out=out)
                assert st == 0, (k, st)
                data = owned_bytes(c, raw) if c["hash_owned"] else raw.tobytes()
                nonzero = nonzero or any(owned_bytes(c, raw) if c["own"] is not None else data)
                h.update(data)
            for v in range(c["n_out"]):
                h.update(bytes(e.overflow(v)))
            path = None
            if native:
                if c["rt"]:
                    graph = e.rt_stats()["graph"]
                    e.rt_end()
                else:
                    graph = 0
                    e.sync()
                path = [int(e.block_mode), bool(e.uses_wave_fft), int(e.output_lag), int(graph)]
        finally:
            if native:
                e.close()
    return h.hexdigest(), bool(nonzero), path


def run_case(c, engine_cls=None):
    """-> {"sha256", "sha256_off", "nonzero", "path"}"""
    if engine_cls is None:
        import brutefir_amd as bf
        engine_cls = bf.Engine
    sha, nonzero, path = run_one(c, c, engine_cls)
    sha_off, nonzero_off, _ = run_one(neutral(c), c, engine_cls)
    return {"sha256": sha, "sha256_off": sha_off, "nonzero": nonzero and nonzero_off, "path": path}


def shows_its_branch(c, got):
    if c["want_mode"] is not None and got["path"] is not None and got["path"][0] != c["want_mode"]:
        return False
    return (got["sha256"] == got["sha256_off"]) == bool(c["transparent"])


def main(argv):
    out = None
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    oracle = "--oracle" in argv
    argv = [a for a in argv if a != "--oracle"]
    cs = case_list()
    names = argv or list(cs)
    engine_cls = None
    if oracle:
        import bforacle
        engine_cls = bforacle.Engine
        names = [n for n in names if oracle_can(cs[n])]
    res = {}
    for n in names:
        res[n] = run_case(cs[n], engine_cls)
        print(n, res[n], file=sys.stderr, flush=True)
        assert res[n]["nonzero"] and shows_its_branch(cs[n], res[n]), (n, res[n])
    text = json.dumps(res, indent=1, sort_keys=True) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
