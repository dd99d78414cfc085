"""The teacher-forced block oracle (tests/step_block_oracle.py) itself, without a GPU: that it restates the step
oracle/resnet_oracle.py computes (self-consistency), that its noise floors are finite and ordered, that the bars of
tests/test_gpu_step_blocks.py catch a subtly wrong block in the block it belongs to and nowhere else (seeded faults), and
that the GPU case list reaches every route of the table (io_net_step_routes on 256 CUs; host arithmetic)."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_block_oracle as sbo
import step_route_inputs as sri
from helpers import orc, synthetic
from instaorder_amd import _lib, engine

N, S = 4, 64
FAULT_BLOCKS = (1, 3, 14)                    # a layer-1 block, a stride-2 block, a layer-4 block


def inputs(heads, seed=11):
    sd = synthetic.make_state_dict(seed, 5, heads, style="kaiming")
    b = synthetic.make_pair_batch(seed + 1, N, S)
    x = torch.from_numpy(np.concatenate([b["modal1"], b["modal2"], b["rgb"]], 1)).double()
    k = sum(heads) if isinstance(heads, list) else heads
    dl = torch.randn(N, k, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64) * 0.01
    return sd, x, dl


def resnet_oracle_step(sd, x, dl, G):
    """oracle/resnet_oracle.py's own fp64 training forward (its _bn / _bottleneck, one call per sample group as loss_o
    makes them), the tensors the step keeps, and its plain autograd gradients"""
    state = orc.state_from_numpy(sd)
    names = orc.param_names(state)
    for k in state:
        if state[k].dtype == torch.float32:
            state[k] = state[k].double()
    for k in names:
        state[k].requires_grad_(True)
    per_group = []
    for xg in x.chunk(G):
        acts = [torch.nn.functional.conv2d(xg, state["conv1.weight"], stride=2, padding=3)]
        h = torch.relu(orc._bn(acts[0], state, "bn1", True))
        acts.append(torch.nn.functional.max_pool2d(h, kernel_size=3, stride=2, padding=1))
        for li, bi in sbo.BLOCKS:
            acts.append(orc._bottleneck(acts[-1], state, "layer%d.%d" % (li + 1, bi), 2 if (bi == 0 and li > 0) else 1,
                                        bi == 0, True))
        f = torch.flatten(torch.nn.functional.adaptive_avg_pool2d(acts[-1], 1), 1)
        heads = [("fc_occ", "fc_depth")] if "fc_occ.weight" in state else [("fc",)]
        acts.append(torch.cat([torch.nn.functional.linear(f, state[h + ".weight"], state[h + ".bias"])
                               for h in heads[0]], 1))
        per_group.append(acts)
    acts = [torch.cat(ts, 0) for ts in zip(*per_group)]
    gl = torch.autograd.grad(acts[-1], [state[k] for k in names], dl)
    running = {k: v for k, v in state.items() if k.endswith("running_mean") or k.endswith("running_var")}
    return [a.detach() for a in acts], dict(zip(names, gl)), running


@pytest.mark.parametrize("heads", [2, [2, 3]], ids=["heads2", "heads2_3"])
@pytest.mark.parametrize("G", [1, 2])
def test_self_consistency_with_resnet_oracle(heads, G):
    sd, x, dl = inputs(heads)
    acts, grads, running = resnet_oracle_step(sd, x, dl, G)
    o = sbo.run(sbo.state64(sd), x, dl, G, stored=acts)
    fwd, ge, re = sbo.errors(acts, grads, running, o)
    assert len(fwd) == sbo.NUNITS and max(fwd) < 1e-12, fwd
    assert set(ge) == set(grads) and max(ge.values()) < 1e-10, max(ge.items(), key=lambda t: t[1])
    assert max(re.values()) < 1e-12, max(re.items(), key=lambda t: t[1])
    # the free run is the same step
    free = sbo.run(sbo.state64(sd), x, dl, G)
    assert max(sbo.err_max(a, r) for a, r in zip(free["acts"], acts)) < 1e-12
    assert max(sbo.err_l2(free["grads"][k], grads[k]) for k in grads) < 1e-10


@pytest.fixture(scope="module")
def bench():
    """heads [2, 3], G = 2: the exact step, the oracle on its stored tensors, and the noise floors of both dtypes"""
    sd, x, dl = inputs([2, 3])
    state = sbo.state64(sd)
    exact = sbo.run(state, x, dl, 2)
    clean = sbo.run(state, x, dl, 2, stored=exact["acts"], track=True)
    ec = {dt: sbo.noise_floor(state, x, dl, 2, dt) for dt in ("fp32", "bf16")}
    return state, x, dl, exact, clean, ec


@pytest.mark.parametrize("G", [1, 2])
def test_noise_floors_are_finite_and_ordered(bench, G):
    state, x, dl = bench[:3]
    ec = bench[5] if G == 2 else {dt: sbo.noise_floor(state, x, dl, G, dt) for dt in ("fp32", "bf16")}
    f32, b16 = ec["fp32"], ec["bf16"]
    for u in range(sbo.NUNITS - 1):
        assert 0 < f32[0][u] < b16[0][u] < 1.0, (sbo.UNIT_NAMES[u], f32[0][u], b16[0][u])
    for part in (1, 2):
        for k in f32[part]:
            a, b = f32[part][k], b16[part][k]
            if sbo.block_of(k) == sbo.NUNITS - 1:
                # avgpool + heads round nothing (pooled features, logits and dlogits stay exact): no floor in either
                assert a < 1e-12 and b < 1e-12, (k, a, b)
            else:
                assert np.isfinite(a) and np.isfinite(b) and 0 <= a < b < 1.0, (k, a, b)
    assert f32[0][-1] < 1e-12 and b16[0][-1] < 1e-12
    for name, e in (("fp32", f32), ("bf16", b16)):
        print("%s floors at 4 x 64^2, G = %d: forward max %.2e, gradients max %.2e (%s), running max %.2e"
              % (name, G, max(e[0]), max(e[1].values()), max(e[1], key=e[1].get), max(e[2].values())))


def _fwd_bars(ec, dt):
    return [sbo.bar(ec[dt][0][u], sbo.floor_fwd(dt, u)) for u in range(sbo.NUNITS)]


def _grad_bars(ec, dt):
    return {k: sbo.bar(v, sbo.FLOOR_F32) for k, v in ec[dt][1].items()}


@pytest.mark.parametrize("block", FAULT_BLOCKS)
@pytest.mark.parametrize("fault", ["no_identity", "swap_group_stats", "no_relu"])
def test_seeded_forward_fault_is_caught_in_its_block_only(bench, fault, block):
    state, x, dl, exact, clean, ec = bench
    bad = sbo.run(state, x, dl, 2, fault=(fault, block), backward=False)        # the "kernel": one block wrong
    o = sbo.run(state, x, dl, 2, stored=bad["acts"], backward=False)
    fwd = sbo.errors(bad["acts"], None, None, o)[0]
    for dt in ("fp32", "bf16"):
        bars = _fwd_bars(ec, dt)
        for u in range(sbo.NUNITS):
            if u == 2 + block:
                assert fwd[u] > bars[u], (dt, fault, sbo.UNIT_NAMES[u], fwd[u], bars[u])
            else:
                assert fwd[u] < bars[u], (dt, fault, sbo.UNIT_NAMES[u], fwd[u], bars[u])


@pytest.mark.parametrize("block", FAULT_BLOCKS)
@pytest.mark.parametrize("fault", ["drop_residual_grad", "shift_mask", "dgamma3_unmasked", "wgrad_over_G"])
def test_seeded_backward_fault_is_caught_where_it_belongs(bench, fault, block):
    """A backward fault is carried upstream by the gradient itself, so "nowhere else" means: nothing behind the block
    (larger index) and nothing beside it.  A dropped residual gradient is the gradient of the PREVIOUS block's output: it
    shows there first.  dgamma and the filter-gradient scale leave the data gradient alone: only their own tensors.

    At the fp32 bar every fault is caught exactly there.  THE LIMIT OF THE bf16 GRADIENT BAR: the gradient is not
    teacher-forced, and the inner ReLU masks of a bf16 step differ from the exact ones on the ~0.3 % of elements within a
    rounding of zero, in every block behind the one looked at; at 4 x 64^2 that puts ec of layer 4's tensors at 0.04 .. 0.1
    and of layer 1's at 0.2, the bars at 0.15 .. 0.65.  So at the bf16 bar: never a false alarm, and a fault is seen in its
    own block wherever its size is above that block's bar -- always in layer 4, a shifted mask and an unmasked dgamma
    everywhere; a filter gradient scaled by 1 / 2 (error 0.5 exactly) in layer 1 or 2, or a residual gradient dropped in
    front of layer 1's first block, is not (the figures are printed)."""
    state, x, dl, exact, clean, ec = bench
    bad = sbo.run(state, x, dl, 2, stored=exact["acts"], fault=(fault, block))
    ge = sbo.errors(None, bad["grads"], None, clean)[1]
    p = sbo.UNIT_NAMES[2 + block]
    layer = p.split(".")[0]
    if fault == "dgamma3_unmasked":
        want, first = {p + ".bn3.weight"}, None
    elif fault == "wgrad_over_G":
        want, first = {k for k in ge if k.startswith(layer + ".") and (".conv" in k or "downsample.0" in k)}, None
        assert all(abs(ge[k] - 0.5) < 1e-9 for k in want)              # 1 - 1 / G, exactly
    else:
        first = 2 + block - (1 if fault == "drop_residual_grad" else 0)
        want = {k for k in ge if sbo.block_of(k) == first}
    # the fp32 comparison of tests/test_gpu_step_blocks.py lets the oracle take the step's decision where an inner ReLU input
    # lies within fp32 rounding of zero: the faults must stay caught through that
    res, nund, _ = sbo.resolve_undecided(clean, bad["grads"], lambda tg: sbo.run(state, x, dl, 2, stored=exact["acts"],
                                                                                 track=True, toggle=tg))
    assert nund > 0
    ge32 = sbo.errors(None, bad["grads"], None, res)[1]
    for dt in ("fp32", "bf16"):
        bars = _grad_bars(ec, dt)
        over = {k for k in ge if (ge32 if dt == "fp32" else ge)[k] > bars[k]}
        allowed = want if first is None else {k for k in ge if sbo.block_of(k) <= first}
        assert over <= allowed, (dt, fault, block, sorted(over - allowed))
        if dt == "fp32" or block == FAULT_BLOCKS[-1]:
            if first is None or fault == "shift_mask":                 # every tensor named sees the fault
                assert want <= over, (dt, fault, block, sorted(want - over))
            else:
                assert want & over, (dt, fault, block)
        else:
            assert over >= {k for k in want if ge[k] > bars[k]}
            print("bf16 bar, %s at %s: caught in %d of its %d own tensors" % (fault, p, len(want & over), len(want)))


def test_undecided_inner_masks_are_read_off_the_step_and_nothing_else_is(bench):
    """An fp32 step may take an inner ReLU either way where its input lies within fp32 rounding of zero, and one such
    element moves every gradient upstream by ~1e-3.  resolve_undecided finds the step's decisions from its BatchNorm bias
    gradients and the oracle then agrees exactly; a decision that is NOT within rounding of zero stays an error."""
    state, x, dl, exact, clean, ec = bench
    bars = _grad_bars(ec, "fp32")
    und = [(k, v[0]) for k, v in clean["undecided"].items() if len(v[0]) and float(v[3].abs().max()) > 0]
    assert len(und) >= 2, "no undecided element with a gradient at this shape"
    rerun = lambda tg: sbo.run(state, x, dl, 2, stored=exact["acts"], track=True, toggle=tg)      # noqa: E731
    step = sbo.run(state, x, dl, 2, stored=exact["acts"], toggle={und[0][0]: und[0][1], und[-1][0]: und[-1][1][:1]})
    before = sbo.errors(None, step["grads"], None, clean)[1]
    assert max(before.values()) > 10 * max(bars.values())
    res, nund, ntog = sbo.resolve_undecided(clean, step["grads"], rerun)
    after = sbo.errors(None, step["grads"], None, res)[1]
    assert ntog >= 1 and max(after.values()) < 1e-10, (ntog, max(after.values()))
    # a step that is right everywhere: nothing is toggled
    assert sbo.resolve_undecided(clean, clean["grads"], rerun)[2] == 0
    # the element of the same BatchNorm closest to zero but OUTSIDE the bound, taken the wrong way: not absorbed
    name, idx = und[0]
    full = sbo.run(state, x, dl, 2, stored=exact["acts"], track=True)
    wide = None
    orig = sbo.UNDECIDED
    try:
        sbo.UNDECIDED = orig * 64
        wide = sbo.run(state, x, dl, 2, stored=exact["acts"], track=True)["undecided"][name]
    finally:
        sbo.UNDECIDED = orig
    outside = [int(u) for u, g in zip(wide[0], wide[3]) if int(u) not in set(idx.tolist()) and abs(float(g)) > 0]
    assert outside, "no element between 1x and 64x the bound"
    wrong = sbo.run(state, x, dl, 2, stored=exact["acts"], toggle={name: torch.tensor(outside[:1])})
    res, _, _ = sbo.resolve_undecided(full, wrong["grads"], rerun)
    err = sbo.errors(None, wrong["grads"], None, res)[1]
    assert any(err[k] > bars[k] for k in err), max(err.values())


def _table(net, case, ncu):
    dt, n, s, G, mode, xop = case
    out = (C.c_int32 * 16)()
    r = _lib.lib().io_net_step_routes(net.handle, n, s, G, mode, xop, ncu, out, 16)
    assert r == 16, (r, _lib.last_error())
    return [int(w) for w in out]


def test_gpu_case_list_reaches_every_route():
    nets = {dt: engine.Net(5, [2, 3], dt) for dt in ("fp32", "bf16")}
    seen = {}
    layer_of = [li + 2 - 1 for li, _ in sbo.BLOCKS]                   # 1 .. 4
    x3p_layers, r2_layers, x1s_blocks, f3_only = set(), set(), set(), False
    for case in sbo.CASES:
        dt, n, s, G, mode, xop = case
        words = _table(nets[dt], case, sbo.CASE_NCU)
        want = sri.routes(sri.BF16 if dt == "bf16" else sri.F32, n, s, G, mode, xop, sbo.CASE_NCU)
        assert words == [sri.pack(r) for r in want], sbo.case_id(case)
        for i, w in enumerate(words):
            r = sri.unpack(w)
            for k in sri.FIELDS + ("out_route",):
                seen.setdefault(k, set()).add(r[k])
            if r["x3p"]:
                x3p_layers.add(layer_of[i])
            if r["out_route"] == 2:
                r2_layers.add(layer_of[i])
            if r["x1s"]:
                x1s_blocks.add(i)
            f3_only = f3_only or (r["f3"] and not r["f2"])
    for k in sri.FIELDS:
        assert seen[k] == {False, True}, (k, seen[k])
    assert seen["out_route"] == {0, 1, 2}
    assert x3p_layers >= {2, 3, 4} and r2_layers >= {2, 3, 4}, (x3p_layers, r2_layers)
    assert len(x1s_blocks) >= 2 and all(sri.BLOCKS[i][1] == 2 for i in x1s_blocks), x1s_blocks
    assert f3_only
