"""The launch sequence of one training step, pinned against the parent commit's: every conv,
BN-apply, BN-reduce and BN-backward-apply launch of a profiled step (forward, loss, backward on
one stream) in issue order with its class, layer, work and bytes as seg_profile_dump prints them,
and the seg_counter values, equal row by row to tests/golden/step_sequence_parent.json
(recorded by tests/golden/make_step_sequence_fixture.py from the library before csrc/net.cpp was
split). A change that moves, adds or drops a launch shows exactly which."""
import json
import os

import pytest

import step_sequence_cases as cases

pytestmark = pytest.mark.gpu

CLASSES = {0: "conv forward", 1: "conv dgrad", 2: "conv wgrad", 3: "BN apply", 4: "BN bwd reduce",
           5: "BN bwd apply"}


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(os.path.dirname(__file__), "golden", "step_sequence_parent.json")) as f:
        fx = json.load(f)
    assert fx["columns"] == ["class", "conv", "work", "bytes"]
    assert list(fx["cases"]) == cases.CASE_NAMES
    return fx["cases"]


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_step_sequence_matches_parent(cuda, parent, name):
    rows, counters, names = cases.record(name)
    want = parent[name]

    def show(r):
        return f"{CLASSES.get(r[0], r[0])} {names[r[1]]} (conv {r[1]}) work {r[2]} bytes {r[3]}"

    for i, (a, b) in enumerate(zip(rows, want["rows"])):
        if a != b:
            print(f"{name}: first differing record {i}:\n  this tree: {show(a)}\n  parent:    {show(b)}")
        assert a == b, (name, i, a, b)
    assert len(rows) == len(want["rows"]), (name, len(rows), len(want["rows"]))
    assert counters == want["counters"], (name, counters, want["counters"])
