"""AddLossModule's lookup route, library call for library call (no GPU): what the module hands okge_train_forward_backward,
okge_n3_forward_backward and okge_rescale_gradients -- scalars, flags, struct fields, WHICH tensor every pointer names -- and what
it allocates, wraps and leaves in .grad, against the trace tools/record_dropin_calls.py recorded from the commit before the
module's two copies of the route became one (tests/golden/dropin_calls.json).  Exact, and the same trace with FAST_CALL on and
off: the switch chooses persistent or fresh argument structs and nothing else."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_dropin_calls as rec  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "dropin_calls.json")) as f:
    GOLDEN = json.load(f)


def test_every_configuration_is_pinned():
    assert sorted(GOLDEN) == sorted(rec.CONFIGS)


@pytest.mark.parametrize("fast", [True, False], ids=["persistent", "fresh"])
@pytest.mark.parametrize("name", list(rec.CONFIGS))
def test_module_issues_the_recorded_calls(name, fast):
    trace, persistent = rec.record_one(name, fast)
    got = json.loads(json.dumps(trace))                               # (tuples -> lists, as the file holds them)
    want = GOLDEN[name]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert [c["call"] for c in g["lib"]] == [c["call"] for c in w["lib"]], (name, i)
        assert g == w, (name, i)
    # the persistent structs exist only where they were used: never with the switch off, nor under OKGE_VALIDATE
    assert persistent == (fast and not rec.CONFIGS[name].get("validate"))
