"""The block passes (csrc/passes.hip: which kernel runs for a pass of a block, with which arguments) launch
what bfhip.hip launched before they moved.

tools/pass_bits.py hashes the output blocks of a fixed case list from seeded inputs; it was run on the
commit before the move (851e57b) and its result committed as tests/golden/pass_bits_parent.json.  The same
hashes and paths are asserted here.  mac_bits, plan_bits and channel_bits pin the MAC variants, the plans
and the channel stage; these pin which transform path (LDS, wave, big) feeds which schedule and entry
point: block_dev in order (f32 and f64), the phase calls, the fused outputs_inputs call, the pipelined,
deferred and ping-pong schedules, a four-chunk plan (the in-place sum of do_outputs and of block_owed),
block pairs, the level kernels, real-time mode with graph replay, and the coefficient kernels.

Twins: cases the parent run showed to hash equal (the schedules of one transform path; pairs and single
blocks) are asserted equal here as well, through the hash both share with the golden file and directly in
test_twins_hash_equal_in_the_golden_file."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pass_bits  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pass_bits_parent.json")))
CASES = pass_bits.case_list()
_got = {}


def _run(name):
    if name not in _got:
        _got[name] = pass_bits.run_case(CASES[name])
    return _got[name]


def test_the_case_list_is_the_golden_one():
    assert sorted(CASES) == sorted(GOLDEN)
    for name, c in CASES.items():
        assert GOLDEN[name]["nonzero"] and pass_bits.shows_its_branch(c, GOLDEN[name]), name


def test_twins_hash_equal_in_the_golden_file():
    twins = {n: c["twin"] for n, c in CASES.items() if c["twin"]}
    assert len(twins) >= 10
    for n, t in twins.items():
        assert GOLDEN[n]["sha256"] == GOLDEN[t]["sha256"], (n, t)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_parent_commit(name):
    got = _run(name)
    print(name, got)
    assert got["nonzero"]
    assert pass_bits.shows_its_branch(CASES[name], got)
    assert got["path"] == GOLDEN[name]["path"]
    assert got["sha256"] == GOLDEN[name]["sha256"]
    twin = CASES[name]["twin"]
    if twin:
        assert got["sha256"] == _run(twin)["sha256"], twin
