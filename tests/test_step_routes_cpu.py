"""The route table of the training step (csrc/net.hip plan_routes, read through io_net_step_routes) against the independent
restatement of the rules it replaced (tests/step_route_inputs.py), row by row, and the workspace layout against the values
recorded before the table existed (tests/golden/step_launch_trace.json, key "layout").  Host arithmetic only: no GPU."""
import ctypes as C
import json
import os

import pytest

import step_route_inputs as sri
from instaorder_amd import _lib, engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_launch_trace.json")
NETS = {}


def net_of(dt):
    if dt not in NETS:
        NETS[dt] = engine.Net(5, [2, 3], "bf16" if dt == sri.BF16 else "fp32")
    return NETS[dt]


def table(dt, N, S, G, mode, xop, ncu):
    out = (C.c_int32 * 16)()
    n = _lib.lib().io_net_step_routes(net_of(dt).handle, N, S, G, mode, xop, ncu, out, 16)
    assert n == 16, (n, _lib.last_error())
    return [int(w) for w in out]


def test_route_table_equals_the_restated_rules_and_reaches_every_arm():
    seen = {}
    ncases = 0
    for case in sri.cases():
        ncases += 1
        want = sri.routes(*case)
        got = table(*case)
        for i, (w, r) in enumerate(zip(got, want)):
            assert w == sri.pack(r), (case, i, sri.unpack(w), r)
            for k, v in r.items():
                seen.setdefault(k, set()).add(v)
    # 2 dtypes x (5 shapes x 3 group counts, less (3, 96) with G = 2, 8 and (4, 64) with G = 8) x 3 x 2 x 2
    assert ncases == 2 * 12 * 12
    # not vacuous: over the set every flag is both set and clear, every output route and every stage occurs
    for k in sri.FIELDS:
        assert seen[k] == {False, True}, (k, seen[k])
    assert seen["out_route"] == {0, 1, 2} and seen["stage"] == {0, 1, 2, 3}


def test_route_table_refuses_what_the_entry_points_refuse():
    lib = _lib.lib()
    out = (C.c_int32 * 16)()
    h = net_of(sri.F32).handle
    assert lib.io_net_step_routes(h, 4, 64, 3, 1, 1, 256, out, 16) < 0          # G does not divide N
    assert lib.io_net_step_routes(h, 4, 72, 1, 1, 1, 256, out, 16) < 0          # S is no multiple of 32
    assert lib.io_net_step_routes(h, 4, 64, 1, 1, 1, 256, out, 15) < 0          # no room for 16 blocks
    assert lib.io_net_step_routes(h, 4, 64, 1, 1, 1, 0, out, 16) < 0            # no CUs


def test_workspace_layout_is_the_recorded_one():
    want = json.load(open(GOLDEN))["layout"]
    assert len(want) == 2 * len(sri.SHAPES)
    for dt, name in ((sri.F32, "fp32"), (sri.BF16, "bf16")):
        net = net_of(dt)
        for N, S in sri.SHAPES:
            got = [net.workspace_bytes(N, S, True), net.workspace_bytes(N, S, False)] + \
                [net.activation_offset(N, S, w) for w in [0] + list(range(2, 19))]
            assert got == want["%s-n%d-s%d" % (name, N, S)], (name, N, S)
