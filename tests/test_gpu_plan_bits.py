"""The plan builder (csrc/plan.hip: host steps over one Plan value, one upload step) builds the plans
the single function before it built.

tools/plan_bits.py hashes the output blocks of a fixed case list from seeded inputs; it was run on the
commit before the split (a55e726) and its result committed as tests/golden/plan_bits_parent.json.  The
same hashes, kernel choices and algorithmic byte counts are asserted here.  The tolerance tests of the
other suites catch a wrong sum; these catch what a reshuffle of the builder can alter below any tolerance:
the order an output's terms are summed in, the chunk split, the path an entry takes.

Every case is f32, L = 512, N = 3 or 4 unless it says otherwise.  Two cases are larger than first
planned, by the least that reaches their branch: an entry is dense only with all OG = 8 terms, so the
shards split 8 outputs (3 inputs, 10 filters), not 4; and powersave's input runs at 0.3 of full scale,
since a window of the usual 0.1 peaks below the noise floor of 0.5 and every block would be silence.
split_along_p is held to the crossbar kernel and to four chunks by BFHIP_MAC_DIAG=0 and
BFHIP_MAC_TARGET_WGS=4: a single 1 x 1 entry would otherwise take the diag kernel, which diag_parts
covers."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import plan_bits  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_bits_parent.json")))
CASES = plan_bits.case_list()


def test_the_case_list_is_the_golden_one():
    assert sorted(CASES) == sorted(GOLDEN)
    for name, c in CASES.items():
        assert plan_bits.shows_its_branch(c, GOLDEN[name]), name
    assert GOLDEN["diag_parts"]["path"][1] is True and GOLDEN["stream_layout"]["path"][2] is True


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_parent_commit(name):
    got = plan_bits.run_case(CASES[name])
    print(name, got)
    assert got["nonzero"]
    assert plan_bits.shows_its_branch(CASES[name], got)
    assert got["path"] == GOLDEN[name]["path"]
    assert got["bytes"] == GOLDEN[name]["bytes"]
    assert got["sha256"] == GOLDEN[name]["sha256"]
