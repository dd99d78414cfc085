"""The training step launches what it launched before its routes moved into one table (csrc/net.hip plan_routes): per
case of tools/step_trace.py the launch list (class, flops, bytes) of forward + backward, and of the backward as one
io_net_backward_stages call per stage, equals the list recorded on the commit before the table
(tests/golden/step_launch_trace.json), and logits and the flat gradient have the recorded SHA-256 wherever that commit
repeated its own bits (every case did).  The record names the CU count it was taken on: routes depend on it."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("step_trace", os.path.join(ROOT, "tools", "step_trace.py"))
step_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(step_trace)

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "step_launch_trace.json")))


def test_every_traced_case_is_recorded():
    assert sorted(GOLDEN["cases"]) == sorted(step_trace.case_id(c) for c in step_trace.CASES)


@pytest.mark.parametrize("case", step_trace.CASES, ids=step_trace.case_id)
def test_step_launches_and_bits_are_the_recorded_ones(case):
    assert step_trace.cu_count() == GOLDEN["cu_count"], \
        "the launch record was taken on %d CUs, this device has %d: routes and grids differ, re-record on this device" % (
            GOLDEN["cu_count"], step_trace.cu_count())
    want = GOLDEN["cases"][step_trace.case_id(case)]
    got = step_trace.run_case(case)
    for k in ("whole", "staged"):
        assert len(got[k]) == len(want[k]), (k, len(got[k]), len(want[k]))
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a == b, "%s: launch %d is %r, recorded %r" % (k, i, a, b)
    for k in ("logits", "grads", "grads_staged"):
        if k in want:
            assert got[k] == want[k], k
