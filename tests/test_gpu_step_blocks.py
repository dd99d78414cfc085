"""Every block of the ResNet-50 training step against the teacher-forced fp64 oracle (tests/step_block_oracle.py), per
route: the case list (step_block_oracle.CASES) reaches every field of the route table on 256 CUs
(tests/test_step_blocks_cpu.py proves it, and that the bars below catch a wrong block in its own block).

Per case, one training forward + backward through resnet_cls.ResNet / engine.Net on kaiming weights (un-damped), a real
pair batch and dlogits ~ 0.01 N(0, 1):
  forward    the stored stem conv output, max-pool output and 16 block outputs (io_net_activation_offset) and the logits,
             each against the unit recomputed in fp64 from ITS stored input: max|got - ref| / max|ref|;
  running    mean / variance of every BatchNorm, likewise (bn1 of the stem, each block's bn1 and downsample BatchNorm read
             a stored tensor: exact up to accumulation);
  gradients  every parameter tensor against the oracle's: L2 relative; the stem filter on its 5 real channels, the 3
             padding channels exactly zero;
  staged     the backward again as one io_net_backward_stages call per stage on a fresh forward: bit-identical flat_grads;
  NaN        logits and flat_grads are filled with NaN before the calls; none may remain in the logits or in any float a
             parameter tensor owns (the alignment gaps of the flat buffer are not gradients and are not written).
Bar of a unit / tensor: 3 x ec + floor, ec = the oracle's emulated run in the case's dtype against its exact run on the
same inputs (CPU only, once per (dtype, N, S, G)), floors 6e-3 (bf16 tensor) / 2e-5 (fp32 tensor or sum) / 1e-5 (logits).
Every unit and every tensor is held to it.

The emulation behind ec models what the step does to a filter and to the statistics (found with this test: with filters
and statistics left exact, bf16 running means sat at 1.5e-3 .. 1.9e-3 against bars of 1e-4): a convolution reads its
filter as a bf16 operand, and BatchNorm statistics are those of the fp32 accumulators (convolutions with the statistics
epilogue: the stem's bn1 differs from the statistics of the stored tensor by exactly the emulation's 3.03e-4 at 4 x 64^2) or
of the rounded tensor in memory (the statistics pass of untiled shapes); ec is the larger of the two emulations'.

Measured on an MI355X, 256 CUs (worst error / bar per case, with the unit or tensor it occurred in):
  case                           forward            running                             gradients
  fp32  3 x 96^2  G 1            0.084 layer4.0     0.020 layer4.0.bn2.running_mean     0.186 layer2.0.bn2.weight
  fp32  8 x 64^2  G 1            0.072 layer2.1     0.016 layer4.1.bn2.running_mean     0.198 layer1.2.bn1.bias
  fp32  8 x 64^2  G 2            0.079 layer4.0     0.026 layer4.2.bn1.running_var      0.255 layer1.2.bn1.bias   (1 of 14)
  fp32 32 x 64^2  G 1            0.086 layer3.1     0.012 layer3.4.bn2.running_mean     0.263 layer1.2.bn1.bias   (3 of 62)
  bf16  3 x 96^2  G 1  p256 1    0.306 layer3.1     0.465 layer1.2.bn2.running_var      0.456 layer4.2.bn1.weight
  bf16  4 x 64^2  G 1  p256 0    0.279 layer4.2     0.580 layer3.5.bn1.running_var      0.458 bn1.bias
  bf16  4 x 64^2  G 1  p256 1    0.279 layer4.2     0.580 layer3.5.bn1.running_var      0.458 bn1.bias
  bf16  4 x 64^2  G 1  p256 3    0.304 layer4.0     0.591 layer3.5.bn1.running_var      0.463 bn1.bias
  bf16  4 x 64^2  G 2  p256 3    0.284 layer3.0     0.525 layer4.1.bn1.running_var      0.406 layer1.2.bn1.weight
  bf16 16 x 64^2  G 1  p256 3    0.263 layer1.0     0.388 layer4.2.bn3.running_var      0.391 bn1.bias
  bf16 16 x 64^2  G 2  p256 3    0.259 layer3.0     0.402 layer4.1.bn3.running_var      0.365 layer2.0.bn2.bias
  bf16 16 x 64^2  G 1  xop 0     0.263 layer1.0     0.417 layer4.0.bn3.running_mean     0.426 bn1.bias
  bf16 64 x 64^2  G 1  p256 3    0.254 layer1.0     0.370 layer4.1.bn2.running_var      0.403 layer1.1.bn1.bias
Staged and whole gradients are bit-identical in all 13 cases, no NaN remains, forward and running statistics pass in all.

(k of n): inner ReLU inputs within fp32 rounding of zero, and how many of them the step took the other way than the
oracle's recomputation (0 of 17 and 0 of 16 in the first two fp32 cases).  Such an element is undecidable for the oracle --
either sign is a correct fp32 result -- and ONE of them moves every gradient upstream of it by ~1e-3: held to its own inner
masks the oracle put 57 of 163 tensors of these two cases at 5e-4 .. 8e-3 against bars of 2.1e-5 (176 and 402 times the
bar), everything from layer2.2's conv1 / bn1 upstream.  At 8 x 64^2, G = 2 the smallest |bn1(y1)| of layer2.2 is 1.09e-6
(typical 0.8, the next 3.1e-5); taking exactly that element the other way reproduced all 57 measured errors to within
0.6 % and left the other 106 below 2e-7.  So in fp32 the oracle takes the step's decision at those elements, and only there
(step_block_oracle.resolve_undecided: read off the BatchNorm bias gradient, as the block-output masks are read off the
stored outputs; tests/test_step_blocks_cpu.py shows that a decision outside the rounding bound is not absorbed and that
every seeded fault stays caught).  In bf16 such elements are 0.3 % of all, and part of ec."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import step_block_oracle as sbo
from helpers import synthetic
from instaorder_amd import _lib, engine, resnet_cls

pytestmark = pytest.mark.gpu

HEADS = [2, 3]
SEED = 211
_CACHE = {}


def _state_dict():
    if "sd" not in _CACHE:
        _CACHE["sd"] = synthetic.make_state_dict(SEED, 5, HEADS, style="kaiming")
        _CACHE["state"] = sbo.state64(_CACHE["sd"])
    return _CACHE["sd"], _CACHE["state"]


def _net(dtype):
    """one module per dtype; the seeded state (running estimates 0 / 1 included) is loaded afresh for every case"""
    sd, _ = _state_dict()
    if ("net", dtype) not in _CACHE:
        _CACHE["net", dtype] = resnet_cls.ResNet(5, HEADS, dtype=dtype).cuda()
    net = _CACHE["net", dtype]
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    net.train()
    return net


def _inputs(dtype, N, S):
    """x8 on the device (the packed input as the step reads it), the same values as float64 NCHW, dlogits"""
    key = ("in", dtype, N, S)
    if key not in _CACHE:
        b = synthetic.make_pair_batch(SEED + N + S, N, S)
        x5 = torch.from_numpy(np.concatenate([b["modal1"], b["modal2"], b["rgb"]], 1))
        x8 = engine.pack_nchw(x5.cuda(), dtype=dtype)
        assert float(x8[..., 5:].float().abs().max()) == 0.0
        x = x8[..., :5].permute(0, 3, 1, 2).double().cpu().contiguous()
        dl = (torch.randn(N, sum(HEADS), generator=torch.Generator().manual_seed(SEED + N * S)) * 0.01)
        _CACHE[key] = (x8, x, dl)
    return _CACHE[key]


def _noise_floor(dtype, N, S, G):
    """ec: does not depend on the p256 mode / xop, and the code under test plays no part in it"""
    key = ("ec", dtype, N, S, G)
    if key not in _CACHE:
        _, x, dl = _inputs(dtype, N, S)
        _CACHE[key] = sbo.noise_floor(_state_dict()[1], x, dl.double(), G, dtype)
    return _CACHE[key]


def _routes(net, case, ncu):
    dtype, N, S, G, mode, xop = case
    out = (C.c_int32 * 16)()
    r = _lib.lib().io_net_step_routes(net.plan.handle, N, S, G, mode, xop, ncu, out, 16)
    assert r == 16, (r, _lib.last_error())
    return [int(w) for w in out]


def _stored(net, ws, N, S):
    """the 18 kept tensors out of the workspace, NCHW float64 on the host"""
    tdt = engine.TORCH_DTYPE[net.dtype]
    es = 2 if net.dtype == "bf16" else 4
    dims = [(0, S // 2, 64), (2, S // 4, 64)]
    H = S // 4
    for i, (li, bi) in enumerate(sbo.BLOCKS):
        H //= 2 if (bi == 0 and li > 0) else 1
        dims.append((3 + i, H, 256 << li))
    out = []
    for which, H, Cc in dims:
        off = net.plan.activation_offset(N, S, which)
        assert off + N * H * H * Cc * es <= ws.numel()
        t = ws[off:off + N * H * H * Cc * es].view(tdt).view(N, H, H, Cc)
        out.append(t.permute(0, 3, 1, 2).double().cpu().contiguous())
    return out


def _forward(net, x8, N, S, G):
    ws = torch.empty(net.plan.workspace_bytes(N, S, True), dtype=torch.uint8, device=x8.device)
    logits = torch.full((N, net.plan.num_logits), float("nan"), device=x8.device)
    net.plan.forward(net.flat_params, net.flat_running, x8, N, S, G, True, ws, logits)
    torch.cuda.synchronize()
    return ws, logits


def _owned(net):
    """the floats of the flat buffers that belong to a tensor (the stem's padding channels included): the layout aligns the
    heads, and the alignment gaps (62 + 61 floats) are nobody's gradient -- the backward leaves them alone"""
    m = torch.zeros(net.plan.param_floats, dtype=torch.bool, device=net.flat_grads.device)
    for t in net.plan.tensors:
        m[t["offset"]:t["offset"] + t["numel_storage"]] = True
    return m


def _bits(t):
    return t.detach().view(torch.int32)


@pytest.mark.parametrize("case", sbo.CASES, ids=sbo.case_id)
def test_every_block_against_the_fp64_oracle(case):
    dtype, N, S, G, mode, xop = case
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert cu == sbo.CASE_NCU, \
        "the launch record was taken on %d CUs, this device has %d: routes and grids differ, re-record on this device" % (
            sbo.CASE_NCU, cu)
    lib = _lib.lib()
    prev = lib.io_set_bf16_p256(mode), lib.io_set_bf16_p256_xop(xop)
    try:
        net = _net(dtype)
        assert _routes(net, case, cu) == _routes(net, case, sbo.CASE_NCU)
        x8, x, dl = _inputs(dtype, N, S)
        state = _state_dict()[1]
        ec_fwd, ec_grad, ec_run = _noise_floor(dtype, N, S, G)

        # 1. forward; the kept tensors leave the workspace before the backward may reuse it
        ws, logits = _forward(net, x8, N, S, G)
        assert not bool(torch.isnan(logits).any())
        stored = _stored(net, ws, N, S) + [logits.double().cpu()]
        sdv = net.state_dict()
        oracle = sbo.run(state, x, dl.double(), G, stored=stored, track=dtype == "fp32")
        running = {k: sdv[k].detach().double().cpu() for k in oracle["running"]}

        # 4. backward
        dld = dl.cuda()
        net.flat_grads.fill_(float("nan"))
        net.plan.backward(net.flat_params, net.flat_grads, x8, dld, N, S, G, ws, None)
        torch.cuda.synchronize()
        whole = net.flat_grads.clone()
        owned = _owned(net)
        assert not bool(torch.isnan(whole[owned]).any())
        grads = {t["name"]: gv.detach().double().cpu() for (t, _), gv in zip(net._param_list, net._grad_views)}
        t0 = net._param_list[0][0]
        assert t0["name"] == "conv1.weight" and t0["cin_storage"] == 8
        pad = whole[t0["offset"]:t0["offset"] + t0["numel_storage"]].view(64, 7, 7, 8)[..., 5:]
        assert float(pad.abs().max()) == 0.0

        # an inner ReLU whose input lies within fp32 rounding of zero: the oracle takes the step's decision (fp32 only; in
        # bf16 such elements are 0.3 % of all and part of ec)
        nund = ntog = 0
        if dtype == "fp32":
            oracle, nund, ntog = sbo.resolve_undecided(oracle, grads, lambda tg: sbo.run(
                state, x, dl.double(), G, stored=stored, track=True, toggle=tg))

        # 2. - 4. every unit, every running estimate, every parameter tensor under its bar
        e_fwd, e_grad, e_run = sbo.errors(stored, grads, running, oracle)
        assert set(e_grad) == set(grads) and len(e_fwd) == sbo.NUNITS
        wf = sbo.worst_ratio(e_fwd, ec_fwd, lambda u: sbo.floor_fwd(dtype, u))
        wr = sbo.worst_ratio(e_run, ec_run, lambda k: sbo.FLOOR_F32)
        wg = sbo.worst_ratio(e_grad, ec_grad, lambda k: sbo.FLOOR_F32)
        print("%s: worst error / bar: forward %.3f (%s: %.2e / %.2e), running %.3f (%s: %.2e / %.2e), "
              "gradients %.3f (%s: %.2e / %.2e); inner ReLU inputs within fp32 rounding of zero: %d, taken the step's way: %d"
              % (sbo.case_id(case), wf[0], sbo.UNIT_NAMES[wf[1]], wf[2], wf[3], wr[0], wr[1], wr[2], wr[3], wg[0], wg[1],
                 wg[2], wg[3], nund, ntog))
        if os.environ.get("IO_STEP_BLOCKS_DUMP"):          # every figure, one JSON line per case, for a closer look
            with open(os.environ["IO_STEP_BLOCKS_DUMP"], "a") as f:
                f.write(json.dumps(dict(case=sbo.case_id(case), fwd=e_fwd, ec_fwd=ec_fwd, grad=e_grad, ec_grad=ec_grad,
                                        run=e_run, ec_run=ec_run)) + "\n")
        bad = ["fwd %s %.3e > %.3e" % (sbo.UNIT_NAMES[u], e_fwd[u], sbo.bar(ec_fwd[u], sbo.floor_fwd(dtype, u)))
               for u in range(sbo.NUNITS) if not e_fwd[u] < sbo.bar(ec_fwd[u], sbo.floor_fwd(dtype, u))]
        bad += ["running %s %.3e > %.3e" % (k, e_run[k], sbo.bar(ec_run[k], sbo.FLOOR_F32))
                for k in e_run if not e_run[k] < sbo.bar(ec_run[k], sbo.FLOOR_F32)]
        bad += ["grad %s %.3e > %.3e" % (k, e_grad[k], sbo.bar(ec_grad[k], sbo.FLOOR_F32))
                for k in e_grad if not e_grad[k] < sbo.bar(ec_grad[k], sbo.FLOOR_F32)]
        assert not bad, (sbo.case_id(case), len(bad), bad[:24])

        # 5. the backward as one call per stage, on a fresh forward: the same bits
        ws, logits2 = _forward(net, x8, N, S, G)
        assert torch.equal(_bits(logits2), _bits(logits))
        net.flat_grads.fill_(float("nan"))
        for s in range(net.plan.backward_stages):
            net.plan.backward(net.flat_params, net.flat_grads, x8, dld, N, S, G, ws, (s, s + 1))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(net.flat_grads[owned]).any())
        assert torch.equal(_bits(net.flat_grads), _bits(whole))
    finally:
        lib.io_set_bf16_p256(prev[0])
        lib.io_set_bf16_p256_xop(prev[1])
