#!/usr/bin/env python3
"""Registers and steady-loop instruction counts of every MAC kernel, from the compiler's assembly.

    python3 tools/mac_resources.py [--parent OTHER_TREE] > profiles/mac_lean_resources.json

Compiles brutefir_amd/csrc/passes.hip, the unit that launches (and so instantiates) the MAC kernels, for
gfx950 to assembly (device side only; no GPU needed; a tree from before that unit existed: bfhip.hip) and reads, per kernel whose name starts with `mac_`: the register counts and the scratch size from the
kernel metadata, and the instruction mix of its steady loop -- the innermost multiplying loop (label .. backward
branch) that holds the most fused multiply-adds.  With --parent the same is done for another checkout
and the two are put side by side (the format of profiles/mac_refactor_resources.json, plus "loops").
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S"]
COLUMNS = ["vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count"]


def unit(tree):
    src = os.path.join(tree, "brutefir_amd", "csrc", "passes.hip")
    return src if os.path.exists(src) else os.path.join(tree, "brutefir_amd", "csrc", "bfhip.hip")


def assembly(tree):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "unit.s")
        subprocess.check_call([hipcc if os.path.exists(hipcc) else "hipcc"] + FLAGS + [unit(tree), "-o", out])
        return open(out).read()


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    return {n: re.sub(r"^void (bfhip::)?(\(anonymous namespace\)::)?", "", d).split("(")[0] for n, d in zip(names, out)}


def loop_mix(body, pipelined=False):
    """the innermost loop with the most fused multiply-adds -> instruction counts
    (pipelined: every innermost multiplying loop that issues all the loads of three stages itself, in code order --
    a kernel of several passes has one or two per pass)"""
    lines = [ln.split(";")[0].strip() for ln in body]
    label_at = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", ln)] if m}
    loops = []
    for i, ln in enumerate(lines):
        m = re.match(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)", ln) or re.match(r"^s_branch\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            loops.append((label_at[m.group(1)], i))
    FMA = ("v_pk_fma_f32", "v_fma_f32", "v_fma_f64", "v_fmac_f32", "v_fmac_f64")
    has_fma = lambda lp: any(ln.startswith(FMA) for ln in lines[lp[0]:lp[1] + 1])      # noqa: E731
    # innermost among the loops that multiply: no other such loop inside (a cursor's small loop may be)
    inner = [lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] and has_fma(o) for o in loops)]
    found = []
    for a, b in inner:
        ins = [ln.split()[0] for ln in lines[a:b + 1] if ln and not ln.endswith(":") and not ln.startswith(".")]
        fma = sum(1 for x in ins if x.startswith(FMA))
        if not fma:
            continue
        found.append({
            "instructions": len(ins), "valu": sum(1 for x in ins if x.startswith("v_")), "fma": fma,
            "v_pk_fma_f32": sum(1 for x in ins if x.startswith("v_pk_fma_f32")),
            "v_pk_mul_f32": sum(1 for x in ins if x.startswith("v_pk_mul_f32")),
            "v_mul": sum(1 for x in ins if x.startswith(("v_mul_f32", "v_mul_f64"))),
            "agpr_moves": sum(1 for x in ins if x.startswith("v_accvgpr")),
            "v_mov": sum(1 for x in ins if x.startswith(("v_mov_b32", "v_mov_b64"))),
            "v_cndmask": sum(1 for x in ins if x.startswith("v_cndmask")),
            "global_load": sum(1 for x in ins if x.startswith("global_load")),
        })
    if pipelined:
        return [f for f in found if f["global_load"] >= 27]
    # the steady loops issue every load themselves (those that fill and drain a pipeline branch around some);
    # a kernel that runs the wave holding element 0 through a copy of its own has two: the lean one first
    top = max(((f["fma"], f["global_load"]) for f in found), default=None)
    return sorted((f for f in found if (f["fma"], f["global_load"]) == top), key=lambda f: f["valu"])


def kernels(text):
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text.split("amdhsa.kernels:")[1])[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {c: int(re.search(r"\.%s:\s+(\d+)" % c, blk).group(1)) for c in COLUMNS}
        meta[name]["agpr_count"] = int(blk.split("\n")[0])
    lines = text.split("\n")
    start = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"^(_Z\w+):\s*(;.*)?$", ln)] if m}
    names = demangle(sorted(meta))
    out = {}
    for name, row in meta.items():
        if not names[name].startswith("mac_") or name not in start:
            continue
        a = start[name]
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        row = dict(row)
        row["loops"] = loop_mix(lines[a:b])
        if names[name].startswith("mac_la_"):
            row["pipelined_loops"] = loop_mix(lines[a:b], pipelined=True)
        out[names[name]] = row
    return out


def per_stage(rows):
    """vector instructions per stage of the pipelined kernels' leanest and heaviest steady loop (MAC_PIPELINE3
    consumes and issues three stages per trip)"""
    out = {}
    for r in rows:
        for side in ("parent", "new"):
            loops = (r.get(side) or {}).get("loops") or []
            if loops and loops[0]["global_load"] in (27, 33):          # 3 x (1 or 3 ring tiles + 8 coefficient tiles)
                out.setdefault(r["kernel"], {})[side] = [round(loops[0]["valu"] / 3), round(loops[-1]["valu"] / 3)]
    return out


def main(argv):
    new = kernels(assembly(ROOT))
    res = {"flags": "hipcc " + " ".join(FLAGS) + " " + os.path.relpath(unit(ROOT), ROOT),
           "columns": COLUMNS + ["agpr_count", "loops: the steady loops (innermost multiplying loops with the most fused multiply-adds and loads), leanest first"]}
    if "--parent" in argv:
        par = kernels(assembly(argv[argv.index("--parent") + 1]))
        res["kernels"] = [{"kernel": k, "parent": par.get(k), "new": new.get(k)} for k in sorted(set(par) | set(new))]
    else:
        res["kernels"] = [{"kernel": k, "new": new[k]} for k in sorted(new)]
    res["valu_per_stage"] = per_stage(res["kernels"])
    json.dump(res, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
