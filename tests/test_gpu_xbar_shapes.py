"""The standard crossbar engine (BFHIP_LONG_WINDOW=0) held to the float64 network model
(tests/xbar_ref.py) on every FFT path, MAC kernel and plan it has.

Every case asserts the path it is meant to reach (uses_wave_fft, uses_diag_mac, window_blocks() ==
2, one block_mode for the whole run), so that no case passes by taking another one.  Impulse
responses are flat (white noise of unit energy): every partition carries the same weight.

Float outputs: relative RMS error per block and output channel (against 1e-3 of the channel's RMS
for a block that is nearly silent) and per channel over the run, within 1e-5 (float32) and 1e-12
(float64).  Integer outputs: S16 exact except within 0.05 LSB of a rounding threshold, 24 and 32 bit
within 2e-6 of full scale; overflow records and status bits equal to xr.encode's.

    a  lengths 4 ... 1048576 (wave transform forced on at 1024 and 2048), N = 2 ... 5, sets ending
       one tap into their last partition, on a partition boundary, and short (per-term MAC)
    b  unit impulses at frame 0 and frame L - 1 on every FFT path: the outputs carry the scaled taps
       and nothing else, within NOISE * ||h||_2
    c  a network per path class: cascades with channel and filter inputs, a dirac, a multi-output
       filter, a delay clamped to N - 1, scaled and short sets; hard and cross-faded switches,
       in/out scale and fscale changes, exact powersave with the inputs silent for more than N blocks
    d  integer outputs on the multi-kernel (big) transform with clipping and the safety limit
    e  one-to-one plans (mac_diag_kernel): every tile count TL and spectrum split, partition splits
    f  MAC variants only an environment variable selects (BFHIP_MAC_NT=0, BFHIP_MAC_UNROLL=1, 3, 4)"""
import numpy as np
import pytest

import brutefir_amd as bf
import cases
import xbar_ref as xr

pytestmark = pytest.mark.gpu
TOL = {4: 1e-5, 8: 1e-12}
NOISE = {4: 4e-7, 8: 1e-15}             # impulse probes: max |error| / ||h||_2 (seen: 4.2e-8, 1.0e-16)
ENV = ("BFHIP_FFT_WAVE", "BFHIP_DIAG_TSPLIT", "BFHIP_DIAG_SPLIT", "BFHIP_MAC_DIAG", "BFHIP_MAC_NT",
       "BFHIP_MAC_UNROLL", "BFHIP_MAC_TARGET_WGS", "BFHIP_OVERLAP", "BFHIP_DEFER", "BFHIP_TEST_WRAP_PERIODS")
OUTFMT = {4: "FLOAT_LE", 8: "FLOAT64_LE"}


def flat_ir(rng, n):
    return rng.standard_normal(n) / np.sqrt(n)


def build(monkeypatch, spec, env=None, powersave=0.0, ch=None):
    """ch: the channel stage around the network (cases.build_channels, xbar_ref.Channels)"""
    monkeypatch.setenv("BFHIP_LONG_WINDOW", "0")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if ch is not None:
        return cases.build_channels(bf.Engine, spec, ch)
    e = bf.Engine(spec["L"], spec["N"], spec["rs"], spec["n_in"], spec["n_out"])
    e.set_interleaved(0, spec["infmt"])
    e.set_interleaved(1, spec["outfmt"])
    if spec.get("safety_limit"):
        e.set_safety_limit(spec["safety_limit"])
    if powersave:
        e.set_powersave(powersave)
    for taps, scale, nb in spec["coeffs"]:
        e.add_coeff(taps, scale, nb)
    for f in spec["filters"]:
        e.add_filter(**f)
    e.finalize()
    return e


def run(monkeypatch, spec, blocks, actions=None, env=None, powersave=0.0, wave=None, diag=False, ch=None):
    """-> (outputs [frames][O] in the output format's units, status per block, engine); the path is
    asserted on every block.  With a channel stage (ch) the outputs are the raw stream, uint8"""
    e = build(monkeypatch, spec, env, powersave, ch)
    wave = spec["L"] in (4096, 8192) if wave is None else wave
    outs, sts, modes = [], [], set()
    for k, b in enumerate(blocks):
        for a in (actions or {}).get(k, ()):
            cases.act(e, a)
        st, raw = e.block(b)
        sts.append(st)
        outs.append(raw)
        assert (e.uses_wave_fft, e.uses_diag_mac, e.window_blocks) == (wave, diag, 2), k
        modes.add(e.block_mode)
    assert len(modes) == 1, modes
    e.sync()
    if ch is not None:
        return np.concatenate(outs), sts, e
    return xr.decode(np.concatenate(outs), spec["outfmt"], spec["n_out"]), sts, e


def hold_blocks(got, want, L, rs, label=""):
    nblk = len(want) // L
    worst = 0.0
    for c in range(want.shape[1]):
        run_rms = np.sqrt((want[:, c] ** 2).sum())
        err = np.sqrt(((got[:, c] - want[:, c]) ** 2).sum()) / max(run_rms, 1e-300)
        assert err <= TOL[rs], (label, c, err)
        worst = max(worst, err)
        floor = 1e-3 * run_rms / np.sqrt(nblk)
        for k in range(nblk):
            s = slice(k * L, (k + 1) * L)
            err = np.sqrt(((got[s, c] - want[s, c]) ** 2).sum()) / max(np.sqrt((want[s, c] ** 2).sum()), floor, 1e-300)
            assert err <= TOL[rs], (label, k, c, err)
            worst = max(worst, err)
    print("XBS %s rs=%d worst=%.3g" % (label, rs, worst))
    return worst


def model(spec, blocks, actions=None):
    x = xr.decode(np.concatenate(blocks), spec["infmt"], spec["n_in"])
    return xr.Network(spec).output(x, len(blocks), actions)


# ------------------------------------------------------------------ a. lengths

def crossbar_spec(L, N, rs, I, O, seed):
    """I x O crossbar of flat sets; pair (o, i) ends one tap into its last partition ((o + i) % 3 ==
    0), on a partition boundary (1) or is a short set of N - 1 partitions (2): every input meets all
    three kinds within one group of 8 outputs"""
    rng = np.random.default_rng(seed)
    coeffs, filters = [], []
    for o in range(O):
        for i in range(I):
            kind = (o + i) % 3
            n = [(N - 1) * L + 1, N * L, (N - 2) * L + L // 2 + 1][kind]
            coeffs.append((flat_ir(rng, n) / I, 1.0, N - 1 if kind == 2 else 0))
            filters.append(dict(in_ch=[i], out_ch=[o], coeff=len(coeffs) - 1))
    return dict(L=L, N=N, rs=rs, n_in=I, n_out=O, infmt="S24_4LE", outfmt=OUTFMT[rs], coeffs=coeffs, filters=filters)


def generic_mac_entries(spec):
    """the MAC entries of a crossbar spec that take the per-term (generic) path.  launch_plan
    (bfhip.hip) makes one entry per (input ring, group of 8 outputs); an entry whose terms are not
    all coefficient terms of its full partition count (a short set beside a full one) is neither the
    crossbar path (dense = 1), nor a single term (dense = 2 + j), nor a full-length subset (dense = 16):
    it runs the generic loop of mac_xbar_kernel.  -> [(input, group)]"""
    L, N = spec["L"], spec["N"]
    terms = {}
    for f in spec["filters"]:
        taps, _, nb = spec["coeffs"][f["coeff"]]
        P = min(nb if nb > 0 else -(-len(taps) // L), N)
        terms.setdefault((f["in_ch"][0], f["out_ch"][0] // 8), []).append(P)
    return [k for k, ps in terms.items() if len(ps) >= 2 and min(ps) < max(ps)]


LENGTHS = [(1 << lg, rs, None) for lg in range(2, 19) for rs in (4, 8)] + \
    [(1 << 19, 4, None), (1 << 20, 4, None), (1 << 20, 8, None)] + \
    [(L, rs, "1") for L in (1024, 2048) for rs in (4, 8)]


@pytest.mark.parametrize("L,rs,wave", LENGTHS, ids=["L%d-rs%d%s" % (L, rs, "-wave" if w else "") for L, rs, w in LENGTHS])
def test_length_sweep(monkeypatch, L, rs, wave):
    lg = L.bit_length() - 1
    N = 2 if L >= 262144 else 3 + lg % 3
    I, O = (3, 9) if L <= 65536 else (2, 2)
    spec = crossbar_spec(L, N, rs, I, O, seed=lg * 10 + rs)
    assert generic_mac_entries(spec), "no entry reaches the per-term MAC"
    blocks = cases.raw_blocks(lg, 2 * N + 2, L, I, "S24_4LE", amplitude=0.3)
    got, sts, e = run(monkeypatch, spec, blocks, env={"BFHIP_FFT_WAVE": wave} if wave else None,
                      wave=True if wave else None)
    assert sts == [0] * len(blocks)
    e.close()
    hold_blocks(got, model(spec, blocks), L, rs, "a L=%d%s" % (L, " wave" if wave else ""))


# ------------------------------------------------------------------ b. impulse probes

PROBES = [(L, rs, w) for L, w in ((16, None), (512, None), (2048, "1"), (4096, None), (16384, None), (32768, None),
                                  (131072, None), (262144, None)) for rs in (4, 8)]


@pytest.mark.parametrize("L,rs,wave", PROBES, ids=["L%d-rs%d%s" % (L, rs, "-wave" if w else "") for L, rs, w in PROBES])
def test_impulse_probes(monkeypatch, L, rs, wave):
    """input 0 feeds outputs 0 and 1, input 1 outputs 1 and 2 (sets ending mid-partition, scaled
    outputs); a unit impulse at frame 0 of block 1 on input 0, at frame L - 1 of block N + 1 on input
    1.  Every output sample -- the taps, the frames before the impulse and after the set's end, the
    outputs an input does not feed -- within NOISE * ||h||_2 of the exact answer"""
    N = 3
    rng = np.random.default_rng(L + rs)
    n = (N - 1) * L + L // 2 + 1
    coeffs = [(flat_ir(rng, n), 1.0, 0) for _ in range(4)]
    filters = [dict(in_ch=[0], out_ch=[0], coeff=0), dict(in_ch=[0], out_ch=[1], out_scale=[0.5], coeff=1),
               dict(in_ch=[1], out_ch=[1], out_scale=[-0.75], coeff=2), dict(in_ch=[1], out_ch=[2], coeff=3)]
    fmt = OUTFMT[rs]
    spec = dict(L=L, N=N, rs=rs, n_in=2, n_out=3, infmt=fmt, outfmt=fmt, coeffs=coeffs, filters=filters)
    nblk = 2 * N + 3
    x = np.zeros((nblk * L, 2))
    x[L, 0] = 1.0
    x[(N + 2) * L - 1, 1] = 1.0
    blocks = [np.ascontiguousarray(x[b * L:(b + 1) * L].astype(cases.RAW_NP[fmt])) for b in range(nblk)]
    got, sts, e = run(monkeypatch, spec, blocks, env={"BFHIP_FFT_WAVE": wave} if wave else None,
                      wave=True if wave else None)
    assert sts == [0] * nblk
    e.close()
    want = np.zeros_like(got)
    for (o, i, g, c) in ((0, 0, 1.0, 0), (1, 0, 0.5, 1), (1, 1, -0.75, 2), (2, 1, 1.0, 3)):
        t0 = L if i == 0 else (N + 2) * L - 1
        want[t0:t0 + n, o] += g * coeffs[c][0][:len(want) - t0]
    norm = max(np.sqrt((coeffs[c][0] ** 2).sum()) for c in range(4))
    err = np.abs(got - want).max(axis=0) / norm
    quiet = np.abs(got[:L]).max() / norm                         # before the first impulse
    tail = np.abs(got[L + n:(N + 2) * L - 1, 0]).max() / norm      # output 0 after the set's end
    print("XBS b L=%d rs=%d%s err/|h|=%s quiet=%.3g tail=%.3g" % (L, rs, " wave" if wave else "", err, quiet, tail))
    assert err.max() <= NOISE[rs] and quiet <= NOISE[rs] and tail <= NOISE[rs], (err, quiet, tail)
    assert np.abs(got[:(N + 2) * L - 1, 2]).max() <= NOISE[rs] * norm     # output 2: input 0 does not feed it


# ------------------------------------------------------------------ c. networks

def network_spec(L, N, rs, seed):
    """cascades with mixed channel + filter inputs, a dirac clamped from delay N + 3, a multi-output
    filter, a scaled short set and a scaled full one with a delay"""
    rng = np.random.default_rng(seed)
    coeffs = [(flat_ir(rng, N * L) / 2, 1.0, 0) for _ in range(3)] + [(flat_ir(rng, 2 * L), 0.5, 2),
                                                                      (flat_ir(rng, N * L - L // 2 + 1), -2.0, 0)]
    filters = [
        dict(in_ch=[0], coeff=0, out_ch=[2], crossfade=True),                                      # 0
        dict(in_ch=[1], coeff=1, delayblocks=1),                                                   # 1
        dict(in_ch=[0], in_scale=[0.25], in_f=[0, 1], in_fscale=[1.0, -0.5], out_ch=[0], coeff=2,
             crossfade=True),                                                                      # 2
        dict(in_ch=[0, 1], in_scale=[0.5, 0.25], in_f=[1], out_ch=[1], coeff=3),                   # 3
        dict(in_ch=[1], out_ch=[0, 1], out_scale=[0.25, -1.0], coeff=-1, delayblocks=N + 3),       # 4: dirac
        dict(in_ch=[0], out_ch=[2], out_scale=[0.5], coeff=4, delayblocks=2),                      # 5
    ]
    return dict(L=L, N=N, rs=rs, n_in=2, n_out=3, infmt="S24_4LE", outfmt=OUTFMT[rs], coeffs=coeffs, filters=filters)


def network_actions(N):
    s0 = N + 5                                    # inputs silent for blocks s0 ... s0 + N + 1
    return {2: [("coeff", 3, 0)],                 # hard switch
            3: [("coeff", 0, 1)],                 # cross-fade
            4: [("coeff", 2, -1), ("scale", 3, 0, 1, -0.75)],
            5: [("scale", 4, 1, 0, 2.0), ("fscale", 2, 1, 0.3)],
            6: [("coeff", 2, 2), ("fscale", 3, 0, -1.5)],
            s0 + 1: [("coeff", 0, 0)],            # a cross-fade while silent
            s0 + N + 3: [("coeff", 2, 4), ("scale", 5, 0, 0, -1.0)]}, s0


def network_case(monkeypatch, L, rs, env=None, label="c"):
    N = 4
    spec = network_spec(L, N, rs, seed=L + rs)
    actions, s0 = network_actions(N)
    nblk = s0 + 2 * N + 6
    blocks = cases.raw_blocks(L % 97 + rs, nblk, L, 2, "S24_4LE", amplitude=0.3)
    for b in range(s0, s0 + N + 2):
        blocks[b][:] = 0
    got, sts, e = run(monkeypatch, spec, blocks, actions, env, powersave=1.0)
    assert sts == [0] * nblk
    e.close()
    want = model(spec, blocks, actions)
    # N + 1 consecutive all-zero input windows (blocks s0 + 1 ... s0 + N + 1): longer than the ring,
    # so powersave holds every input slot a filter of output 2 reads (filter 0 over N partitions,
    # filter 5 over N - 2 behind its delay of 2) silent in blocks s0 + N and s0 + N + 1; there the
    # output is exactly zero
    assert all(not blocks[b].any() for b in range(s0, s0 + N + 2))
    quiet = slice((s0 + N) * L, (s0 + N + 2) * L)
    assert np.abs(want[quiet, 2]).max() <= 1e-12 * np.abs(want[:, 2]).max()
    assert not got[quiet, 2].any()
    return hold_blocks(got, want, L, rs, "%s L=%d" % (label, L))


NETWORKS = [(L, rs) for L in (16, 512, 4096, 16384) for rs in (4, 8)] + [(131072, 4)]


@pytest.mark.parametrize("L,rs", NETWORKS)
def test_network(monkeypatch, L, rs):
    network_case(monkeypatch, L, rs)


# ------------------------------------------------------------------ d. integer outputs, big transform

@pytest.mark.parametrize("L", [65536, 262144])
@pytest.mark.parametrize("fmt", ["S16_LE", "S24_LE", "S32_LE"])
def test_integer_outputs_on_the_big_transform(monkeypatch, L, fmt):
    """2 x 3, float32: output 1 clips (overflow records), the last block is loud enough to pass the
    safety limit (the status bit)"""
    N, I, O, rs = (3 if L == 65536 else 2), 2, 3, 4
    rng = np.random.default_rng(L % 1000 + len(fmt))
    gains = [0.5, 8.0, 1.0]
    coeffs = [(flat_ir(rng, N * L) * gains[o] / I, 1.0, 0) for o in range(O) for i in range(I)]
    filters = [dict(in_ch=[i], out_ch=[o], coeff=o * I + i) for o in range(O) for i in range(I)]
    spec = dict(L=L, N=N, rs=rs, n_in=I, n_out=O, infmt="S24_4LE", outfmt=fmt, coeffs=coeffs, filters=filters,
                safety_limit=4.0)
    nblk = 2 * N + 2
    blocks = cases.raw_blocks(3, nblk, L, I, "S24_4LE", amplitude=0.1)
    blocks[-1] = (blocks[-1].astype(np.int64) * 60).clip(-(1 << 23), (1 << 23) - 1).astype(np.int32)
    got_raw, sts, e = run(monkeypatch, spec, blocks[:-1])
    sb = xr.FORMATS[fmt][1]
    full = float(1 << (8 * sb - 1))
    y = model(spec, blocks)
    want, ofs, st = xr.encode(y[:-L], fmt, L, safety_limit=4.0)
    assert sts == st == [0] * (nblk - 1)
    assert ofs[1].n_overflows > 0 and ofs[0].n_overflows == 0
    got = np.rint(got_raw * full).astype(np.int64)
    u = y[:-L] * full + 0.5
    near = np.abs(u - np.round(u)) < 0.05
    diff = np.abs(got - want)
    if sb == 2:
        assert diff[~near].max() == 0 and diff.max() <= 1
    else:
        assert diff.max() <= 2e-6 * full, diff.max()
    for c in range(O):
        g = e.overflow(c)
        assert g.n_overflows == ofs[c].n_overflows, c
        assert abs(g.intlargest - ofs[c].intlargest) <= (1 if sb == 2 else 2e-6 * full), c
        if ofs[c].n_overflows:
            assert g.largest == pytest.approx(ofs[c].largest, rel=1e-5), c
        assert g.max == pytest.approx(ofs[c].max, rel=1e-5), c
    # the loud block: past the safety limit on outputs 1 and 2 (the records are the reference's
    # partial conversion there, not compared)
    assert xr.encode(y, fmt, L, safety_limit=4.0)[2][-1] == xr.ST_SAFETY
    assert e.block(blocks[-1])[0] == xr.ST_SAFETY
    e.close()


# ------------------------------------------------------------------ e. one-to-one plans

def diag_tiles(L, rs, tsplit_env):
    """(TL, tsplit) for a one-to-one plan under BFHIP_DIAG_TSPLIT: a copy of diag_geometry in
    passes.hip (the mac_diag_kernel launch), which the engine does not report.  It only turns the
    table below (DIAG: the TL and tsplit each case is meant to reach) into the environment that
    reaches it; if diag_geometry's choice changes, this copy and the table have to follow it"""
    all_tiles = max(1, L // (256 * (2 if rs == 4 else 1)))
    ts = 1
    while ts * 2 <= min(all_tiles, tsplit_env):
        ts *= 2
    while all_tiles // ts > 16:
        ts *= 2
    return min(16, all_tiles // ts), ts


# (rs, L, channels, BFHIP_DIAG_TSPLIT, (TL, tsplit) meant, BFHIP_DIAG_SPLIT); L <= 512 (f32) and
# L <= 256 (f64) hold one tile: TL = 1, tsplit = 1 whatever the job count
DIAG = [(4, 64, 4, None, (1, 1), None), (4, 512, 9, None, (1, 1), None), (4, 1024, 4, 2, (1, 2), None)] + \
    [(4, 8192, 4, t, (16 // t, t), None) for t in (1, 2, 4, 8)] + \
    [(8, 256, 9, None, (1, 1), None), (8, 512, 4, 2, (1, 2), None)] + \
    [(8, 4096, 4, t, (16 // t, t), None) for t in (1, 2, 4, 8)] + \
    [(8, 8192, 4, 8, (4, 8), None)] + [(rs, 2048, 4, None, None, s) for rs in (4, 8) for s in (1, 2, 3, 4)]
assert {d[4] for d in DIAG if d[4]} >= {(16 // t, t) for t in (1, 2, 4, 8)} | {(1, 1), (1, 2)}


@pytest.mark.parametrize("rs,L,C,tsplit,tiles,split", DIAG,
                         ids=["rs%d-L%d-ch%d-t%s-%s-s%s" % d for d in DIAG])
def test_one_to_one_plan(monkeypatch, rs, L, C, tsplit, tiles, split):
    """channel k -> output k through its own set (N = 5: partition splits of 1 ... 4 parts)"""
    N = 5
    rng = np.random.default_rng(L + C + rs)
    coeffs = [(flat_ir(rng, N * L - (k % 2) * (L // 2)), 1.0, 0) for k in range(C)]
    filters = [dict(in_ch=[k], out_ch=[k], coeff=k, out_scale=[1.0 - 0.1 * k]) for k in range(C)]
    spec = dict(L=L, N=N, rs=rs, n_in=C, n_out=C, infmt="S24_4LE", outfmt=OUTFMT[rs], coeffs=coeffs, filters=filters)
    env = {}
    if tsplit is not None:
        env["BFHIP_DIAG_TSPLIT"] = str(tsplit)
    if tiles is not None:
        assert diag_tiles(L, rs, tsplit or 1) == tiles
    if split is not None:
        env["BFHIP_DIAG_SPLIT"] = str(split)
    blocks = cases.raw_blocks(C, 2 * N + 2, L, C, "S24_4LE", amplitude=0.3)
    got, sts, e = run(monkeypatch, spec, blocks, env=env, diag=True)
    assert sts == [0] * len(blocks)
    e.close()
    label = "e L=%d ch=%d" % (L, C) + (" TL=%d tsplit=%d" % tiles if tiles else "")
    hold_blocks(got, model(spec, blocks), L, rs, label + (" split=%d" % split if split else ""))


# ------------------------------------------------------------------ f. environment-only MAC variants

MAC_ENV = [{"BFHIP_MAC_NT": "0"}, {"BFHIP_MAC_UNROLL": "1"}, {"BFHIP_MAC_UNROLL": "3"}, {"BFHIP_MAC_UNROLL": "4"}]


@pytest.mark.parametrize("env", MAC_ENV, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
@pytest.mark.parametrize("rs", [4, 8])
def test_mac_variants_crossbar(monkeypatch, env, rs):
    L, N = 1024, 5
    spec = crossbar_spec(L, N, rs, 3, 9, seed=77 + rs)
    for k in range(len(spec["coeffs"])):                     # dense: no short sets
        taps, _, _ = spec["coeffs"][k]
        spec["coeffs"][k] = (np.resize(taps, N * L) if len(taps) < (N - 1) * L else taps, 1.0, 0)
    blocks = cases.raw_blocks(8, 2 * N + 2, L, 3, "S24_4LE", amplitude=0.3)
    got, sts, e = run(monkeypatch, spec, blocks, env=env)
    assert sts == [0] * len(blocks)
    e.close()
    hold_blocks(got, model(spec, blocks), L, rs, "f xbar %s" % env)


@pytest.mark.parametrize("env", MAC_ENV, ids=lambda d: "-".join("%s=%s" % kv for kv in d.items()))
def test_mac_variants_network(monkeypatch, env):
    network_case(monkeypatch, 1024, 4, env, label="f net %s" % env)
