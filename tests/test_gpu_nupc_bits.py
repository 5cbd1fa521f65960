"""The non-uniform convolver computes what it computed before csrc/nupc.hip was taken apart into the
period schedule (nupc_sched.h), the kernels and their launches (nupc_kernels.h), the audio path (nupc.hip)
and the rewrites (nupc_update.hip).

tools/nupc_bits.py hashes the output periods of a fixed case list from seeded inputs; it was run on the
commit before the move (ee5807d) and its result committed as tests/golden/nupc_bits_parent.json.  The same
hashes are asserted here: plain runs in both precisions with background segments and without, aligned
switches at every kind of fade length, two in a row, staggered switches, a staggered one followed by an
aligned one, a gain-only switch, output gain as a step and as a ramp with a request in mid-ramp, dither,
delay changes across the fragment boundary with mutes, sub-delay, planar buffers, and set rewrites
(synchronous, asynchronous, rendered equaliser curves) switched to.  Each case also shows through the
binding that its branch ran."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nupc_bits  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "nupc_bits_parent.json")))
CASES = nupc_bits.case_list()
_got = {}


def _run(name):
    if name not in _got:
        _got[name] = nupc_bits.run_case(CASES[name])
    return _got[name]


def test_the_case_list_is_the_golden_one():
    assert sorted(CASES) == sorted(GOLDEN)
    for name in CASES:
        assert GOLDEN[name]["nonzero"] and GOLDEN[name]["ran"], name


def test_twins_and_differences_in_the_golden_file():
    twins = {n: c["twin"] for n, c in CASES.items() if c["twin"]}
    assert twins == {"update_coeff_async": "update_coeff"}
    for n, t in twins.items():
        assert GOLDEN[n]["sha256"] == GOLDEN[t]["sha256"], (n, t)
    for n, c in CASES.items():
        if c["differs"]:
            assert GOLDEN[n]["sha256"] != GOLDEN[c["differs"]]["sha256"], (n, c["differs"])
    # no other two cases hash equal: background on and off least of all
    assert len({g["sha256"] for g in GOLDEN.values()}) == len(GOLDEN) - len(twins)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_parent_commit(hip, name):
    got = _run(name)
    print(name, got)
    assert got["nonzero"]
    assert got["ran"]
    assert got["sha256"] == GOLDEN[name]["sha256"]
    twin = CASES[name]["twin"]
    if twin:
        assert got["sha256"] == _run(twin)["sha256"], twin
