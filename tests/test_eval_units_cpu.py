"""CPU guards of tests/test_gpu_eval_units.py (no kernel is launched): the case table of tests/eval_unit_oracle.py reaches
every kernel family and arm it is there for, its inputs discriminate, its bars catch a wrong unit in its own unit, and the
tap layout entry points (io_net_eval_tap_offset / io_net_eval_taps_bytes, which need no device) describe a packed buffer."""
import pytest
import torch

import eval_unit_oracle as euo
import step_block_oracle as sbo
from instaorder_amd import _lib, engine

# the two smallest rectangular cases, one per dtype: (dtype, N, H, W)
FAULT_CASES = {"fp32": ("fp32", 1, 32, 256), "bf16": ("bf16", 2, 32, 256)}
# fault -> the unit it is built into: bias_shift64 needs more than 64 channels, no_relu a conv2, wrong_identity a block
# with a downsample branch, missing_tap_row and swap_hw a 3x3 unit on a map with more than one row
FAULT_UNITS = {"no_eps": "layer2.1.a1", "no_mean": "layer1.1.a2", "bias_shift64": "layer1.0.out", "no_relu": "layer2.1.a2",
               "wrong_identity": "layer2.0.out", "missing_tap_row": "layer1.2.a2", "swap_hw": "layer1.0.a2"}


def test_case_table_reaches_every_named_arm():
    seen = set()
    for dtype, N, H, W, modes, _ in euo.CASES:
        for mode in (modes or (1,)):
            pred = euo.predict(dtype, N, H, W, mode)
            assert len(pred) == 53
            for p in pred:
                seen |= p["tags"]
    missing = [t for t in euo.COVERAGE if t not in seen]
    assert not missing, "no case reaches: %s" % ", ".join(missing)
    # the switch the GPU test flips must move launches: every fp32 case has Winograd units, and none with it off
    for dtype, N, H, W, _, _ in euo.CASES:
        if dtype == "fp32":
            assert euo.wino_units(dtype, N, H, W)
            assert not [p for p in euo.predict(dtype, N, H, W, wino=False) if p["family"].startswith("wino-")]
    # ... and the two p256 modes of a bf16 case must differ in at least one route
    for dtype, N, H, W, modes, _ in euo.CASES:
        if dtype == "bf16":
            a, b = [[p["route"] for p in euo.predict(dtype, N, H, W, m)] for m in modes]
            assert a != b


def test_unit_list_matches_the_executor():
    assert euo.NUNITS == 55 and len(euo.CONV_UNITS) == engine.Net.EVAL_CONVS and euo.NTAPS == engine.Net.EVAL_UNITS
    shp = euo.unit_shapes(2, 64, 96)
    assert shp[0] == (64, 32, 48) and shp[1] == (64, 16, 24) and shp[-1] == (2048, 2, 3)
    g = euo.geometries(2, 64, 96)
    assert g[0] == (2, 64, 96, 8, 64, 7, 7, 2, 3) and g[-1] == (2, 2, 3, 512, 2048, 1, 1, 1, 0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_inputs_discriminate(dtype):
    case = FAULT_CASES[dtype]
    state, x = euo.make_state(*case), euo.make_input(*case)[1]
    for j, bn in enumerate(euo.BN_NAMES):
        C = state[bn + ".weight"].numel()
        c_eps, c_neg, c_zero = euo.edge_channels(j, C)
        assert len({c_eps, c_neg, c_zero}) == 3
        assert abs(float(state[bn + ".running_var"][c_eps]) - euo.EDGE_VAR) < 1e-12 and float(state[bn + ".weight"][c_eps]) != 0
        assert float(state[bn + ".weight"][c_neg]) <= -0.25
        assert float(state[bn + ".weight"][c_zero]) == 0.0
        # the estimates are not the seeded 0 / 1
        assert float(state[bn + ".running_mean"].abs().max()) > 0 and float((state[bn + ".running_var"] - 1).abs().min()) > 0
        for k in (".weight", ".running_mean", ".running_var"):
            assert torch.equal(state[bn + k], state[bn + k].float().double())
    ec, acts = euo.noise_floor(*case)
    ref = euo.reference(state, x, acts)
    for name, r in zip(euo.UNIT_NAMES, ref):
        assert float((r != 0).double().mean()) >= 0.10, name
        assert bool(torch.isfinite(r).all()), name
    # the emulation sits where its model says: one rounding of the storage type per stored tensor, exact logits
    assert max(ec[:-1]) < (1e-2 if dtype == "bf16" else 1e-6) and ec[-1] < 1e-12


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("fault", euo.FAULTS)
def test_bars_catch_a_seeded_fault_in_its_own_unit(dtype, fault):
    case = FAULT_CASES[dtype]
    i = euo.UNIT_NAMES.index(FAULT_UNITS[fault])
    bars = euo.bars(dtype, euo.noise_floor(*case)[0])
    err = euo.faulted_errors(*case, fault, i)
    assert err[i] > bars[i], (fault, euo.UNIT_NAMES[i], err[i], bars[i])
    assert len(err) > 1
    for j, e in err.items():
        if j != i:
            assert e < bars[j], (fault, "leaks into", euo.UNIT_NAMES[j], e, bars[j])


def test_clean_emulation_is_under_every_bar():
    for dtype, case in FAULT_CASES.items():
        ec = euo.noise_floor(*case)[0]
        assert all(e < b for e, b in zip(ec, euo.bars(dtype, ec)))
        assert euo.bars(dtype, ec)[-1] == sbo.bar(ec[-1], sbo.FLOOR_LOGITS)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tap_layout_is_packed_and_aligned(dtype):
    net = engine.Net(5, euo.HEADS, dtype=dtype)
    es = 2 if dtype == "bf16" else 4
    for N, H, W in [(2, 64, 64), (1, 32, 256), (3, 96, 64)]:
        total = net.eval_taps_bytes(N, H, W)
        offs = [net.eval_tap_offset(N, H, W, k) for k in range(euo.NTAPS)]
        assert offs[0] == 0 and all(b > a for a, b in zip(offs, offs[1:])) and all(o % 16 == 0 for o in offs)
        sizes = [N * h * w * C * es for C, h, w in euo.unit_shapes(N, H, W)]
        assert [b - a for a, b in zip(offs + [total], (offs + [total])[1:])] == sizes
        assert sum(sizes) == total
    lib = _lib.lib()
    assert lib.io_net_eval_tap_offset(net.handle, 2, 64, 64, euo.NTAPS) == -1 and _lib.last_error()
    assert lib.io_net_eval_tap_offset(net.handle, 2, 64, 64, -1) == -1
    assert lib.io_net_eval_tap_offset(net.handle, 2, 64, 70, 0) == -1
    assert lib.io_net_eval_taps_bytes(net.handle, 2, 48, 64) == 0 and _lib.last_error()
