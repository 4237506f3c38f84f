"""FusedTrainStep, launch for launch (no GPU): what the step asks of its engine -- method, scalar arguments, WHICH of its tensors
it hands over -- the tensors state_tensors() returns, in order, and what its buffers hold after every step, against the trace
tools/record_lookup_step_calls.py recorded from the commit before the step's state moved into one record per table
(tests/golden/lookup_step_calls.json).  Exact: host-side restructuring of the step must not change one argument."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_lookup_step_calls as rec  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "lookup_step_calls.json")) as f:
    GOLDEN = json.load(f)


def test_every_configuration_is_pinned():
    assert sorted(GOLDEN) == sorted(rec.CONFIGS)


@pytest.mark.parametrize("name", list(rec.CONFIGS))
def test_step_issues_the_recorded_calls(name):
    got = json.loads(json.dumps(rec.record_one(name, rec.CONFIGS[name])))          # (tuples -> lists, as the file holds them)
    want = GOLDEN[name]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert [c["call"] for c in g["calls"]] == [c["call"] for c in w["calls"]], (name, i)
        assert g == w, (name, i)
