"""The channel stage in a unit of its own (csrc/channels.hip behind csrc/channels.h) computes the bits
the code spread over bfhip.hip computed before it.

tools/channel_bits.py hashes the output blocks and the final overflow records of a fixed case list from
seeded inputs; it was run on the commit before the move (c60e535) and its result committed as
tests/golden/channel_bits_parent.json.  The same hashes and paths are asserted here.  The tolerance tests
of the other suites catch a wrong sample; these catch what a move can alter below any tolerance or beside
every sample they look at: the order a shared output's members are mixed in, the slot a delay line is in
after a run-time change, where a dither chain's table walk starts, what a byte another engine owns holds.

Every case is f32, L = 256, N = 2, S24_4LE in, 10 blocks unless tools/channel_bits.py says otherwise.  A
case shows its branch when its hash differs from that of its twin with the channel stage neutralised
(identity maps, no delays, mutes, sub-sample filters or dither).  Departures from the first plan of the
cases, each the least that reaches the branch:
  * wide_deferred and its sharded twin: the planar copies of a wide side move bytes and change none, so
    their twin (BFHIP_WIDE_IO=0) must hash EQUAL; what shows the branch is the path, deferred output, the
    schedule whose fused [K3 | K1] launch the transposes surround.  (That the transposes are launched is
    what the dispatch lists compared for this change show; no query of the C ABI reports it.)
  * the S16_LE cases feed their shared output at 0.3 of full scale through gains of 10 and 12: at the
    usual 0.1 and unit gain nothing clips and every overflow record would be trivial.
  * the dither table is built for a rate of 200, so that its spacing (2000) is passed within the 2560
    frames of a run and every chain's walk wraps once.
  * shard_foreign dithers physical outputs 1 and 2 only, both the owner's: a dithered output of its own
    would give the foreign engine the time-sample buffer the case is there to be without.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import channel_bits  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "channel_bits_parent.json")))
CASES = channel_bits.case_list()


def test_the_case_list_is_the_golden_one():
    assert sorted(CASES) == sorted(GOLDEN)
    for name, c in CASES.items():
        assert GOLDEN[name]["nonzero"] and channel_bits.shows_its_branch(c, GOLDEN[name]), name
    assert GOLDEN["wide_deferred"]["path"][0] == channel_bits.MODE_DEFERRED
    assert GOLDEN["rt_n_to_1"]["path"][3] == 0           # not graphable: every period ran the direct path


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_parent_commit(name):
    got = channel_bits.run_case(CASES[name])
    print(name, got)
    assert got["nonzero"]
    assert channel_bits.shows_its_branch(CASES[name], got)
    assert got["path"] == GOLDEN[name]["path"]
    assert got["sha256_off"] == GOLDEN[name]["sha256_off"]
    assert got["sha256"] == GOLDEN[name]["sha256"]
