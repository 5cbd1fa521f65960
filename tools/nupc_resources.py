#!/usr/bin/env python3
"""Registers, LDS, scratch and occupancy of every kernel of the non-uniform convolver, from the compiler's
own report.

    python3 tools/nupc_resources.py [--parent OTHER_TREE] > profiles/nupc_refactor_resources.json
    python3 tools/nupc_resources.py --eq-base > profiles/nupc_eq_base_resources.json

Compiles brutefir_amd/csrc/nupc.hip, the unit that launches (and so instantiates) the nupc kernels, for
gfx950 with -Rpass-analysis=kernel-resource-usage (device side only; no GPU needed) and reads the remarks of
every kernel whose name starts with `nupc_`.  With --parent the same is done for another checkout and the two
are put side by side; "same" says whether every figure of every kernel is equal.  With --eq-base the unit is
brutefir_amd/csrc/nupc_update.hip and the kernels are those of eq_apply.h (the render onto a base), whose names
start with `eq_apply_`; with --biquads the kernels are those of eq_biquad.h (the section render, `bq_`);
with --limiter the unit stays nupc.hip and the kernels are the limiter's two (`nupc_limit_`), the true-peak
instantiations of the limit kernel (third template argument true) beside the sample-peak ones:

    python3 tools/nupc_resources.py --biquads > profiles/nupc_biquads_resources.json
    python3 tools/nupc_resources.py --limiter [--parent OTHER_TREE] > profiles/nupc_truepeak_resources.json"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
         "-Rpass-analysis=kernel-resource-usage"]
COLUMNS = ["VGPRs", "AGPRs", "TotalSGPRs", "LDS Size [bytes/block]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill",
           "Occupancy [waves/SIMD]"]


def kernels(tree, unit="nupc.hip", prefix="nupc_"):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(tree, "brutefir_amd", "csrc", unit)
    err = subprocess.run([hipcc if os.path.exists(hipcc) else "hipcc"] + FLAGS + [src, "-o", os.devnull],
                         capture_output=True, text=True, check=True).stderr
    raw, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", ln)
        if m:
            cur = raw.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][A-Za-z \[\]/]+): (\S+)", ln)
        if m and cur is not None and m.group(1).strip() in COLUMNS:
            cur[m.group(1).strip()] = int(m.group(2))
    names = sorted(raw)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, plain):
        d = re.sub(r"^void |\(anonymous namespace\)::|\w+::", "", d).split("(")[0]      # without namespaces and parameters
        if d.startswith(prefix):
            out[d] = raw[n]
    return out


def main(argv):
    unit, prefix = ("nupc_update.hip", "eq_apply_") if "--eq-base" in argv else \
                   ("nupc_update.hip", "bq_") if "--biquads" in argv else \
                   ("nupc.hip", "nupc_limit_") if "--limiter" in argv else ("nupc.hip", "nupc_")
    new = kernels(ROOT, unit, prefix)
    res = {"flags": "hipcc " + " ".join(FLAGS) + " brutefir_amd/csrc/" + unit, "columns": COLUMNS}
    if "--parent" in argv:
        par = kernels(argv[argv.index("--parent") + 1], unit, prefix)
        res["kernels"] = [{"kernel": k, "parent": par.get(k), "new": new.get(k)} for k in sorted(set(par) | set(new))]
        res["same"] = par == new
    else:
        res["kernels"] = [{"kernel": k, "new": new[k]} for k in sorted(new)]
    json.dump(res, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
