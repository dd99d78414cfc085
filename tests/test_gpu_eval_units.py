"""Every unit of the ResNet-50 INFERENCE forward (run_forward_eval of csrc/net.hip: fold_bn_kernel, then 53 convolutions with
bias (+ identity) (+ ReLU) epilogues on whatever kernel family io_launch_conv_nt picks, height and width carried
separately) against the teacher-forced fp64 oracle of tests/eval_unit_oracle.py, per case of its table
(tests/test_eval_units_cpu.py proves that the table reaches every family and arm it names and that the bars catch a seeded
fault in its own unit).

Per case, through resnet_cls.ResNet and engine.Net.forward_eval_taps (io_net_forward_eval_taps) on kaiming weights with
running estimates at which the fold matters, taps and logits pre-filled with NaN:
  units      the 54 tapped tensors and the logits, each against the unit recomputed in fp64 from ITS tapped input and the
             raw, unfolded parameters: max|got - ref| / max|ref| under 3 x ec + floor (ec: the oracle's emulation of the
             dtype against its exact run, CPU only; floors 6e-3 bf16 tensor / 2e-5 fp32 tensor / 1e-5 logits);
  NaN        none remains in any tap or logit;
  routes     io_debug_last_nt_route after each of the 53 launches equals the prediction (fp32: 0 throughout -- Winograd,
             stem_rows and conv_nt_kernel all report 0; bf16: stem_halo 3, conv_halo3 2, conv_p256 1);
  fp32       again with io_set_winograd(0): under the same bars, every unit before the first predicted-Winograd launch
             bit-identical between the two runs and that unit different (the forward runs free, so everything after the
             first Winograd unit reads different bits in the two runs; its form cannot be isolated further);
  bf16       both io_set_bf16_p256 modes of the case;
  identity   a second tapped run and the plain entry point (io_net_forward_eval_hw, or io_net_forward for H = W, through
             ResNet.forward_packed) give bit-identical logits.
test_orig_mode_driver_in_bf16: inference.orig_mode_inputs -> infer_order_batched with dtype='bf16' on the 131 x 102
scene of tests/test_gpu_datasets.py (a 128 x 96 input), against the fp64 oracle and the fp32 run.

Measured on an MI355X, 256 CUs (worst error / bar per case, with the unit it occurred in):
  case                     first run                              second run
  fp32  2 x  64 x  64      0.095 layer1.1.a2   (Winograd on)      0.102 layer3.4.a2   (Winograd off)
  fp32  1 x  32 x 256      0.080 layer4.2.a1                      0.060 layer3.5.a1
  fp32  4 x  96 x  64      0.110 layer1.2.a2                      0.069 layer4.0.a2
  fp32  8 x  32 x  64      0.127 layer2.3.a2                      0.098 layer4.0.a2
  fp32 17 x 128 x 128      0.113 layer1.2.a2   (12 units)         0.049 layer1.0.a2
  bf16  2 x  32 x 256      0.262 layer3.1.a1   (p256 mode 3)      0.262 layer3.1.a1   (mode 0)
  bf16  2 x  64 x 128      0.274 layer3.2.a2   (p256 mode 3)      0.274 layer3.2.a2   (mode 0)
  bf16  3 x  64 x  64      0.272 layer4.0.a1   (p256 mode 3)      0.272 layer4.0.a1   (mode 1)
fp32 errors are 1.0e-6 .. 2.6e-6 against bars of 2.0e-5 (the Winograd units lead wherever the form runs), bf16 errors
3.8e-3 .. 4.6e-3 against bars of 1.4e-2 .. 1.7e-2.  Every case passed on its first run with the routes as predicted: the eval
executor and the epilogues it reaches have no defect at these shapes.  Driver check: bf16 logits 9.7e-3 from the fp64
oracle (bar 1e-2; the fp32 run 1.2e-6), all 12 decisions outside the bar and equal to the fp32 run's."""
import numpy as np
import pytest
import torch

import eval_unit_oracle as euo
import step_block_oracle as sbo
from helpers import synthetic
from instaorder_amd import _lib, engine, resnet_cls

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture
def switches():
    """the two process-wide switches the cases flip, put back whatever the test does"""
    lib = _lib.lib()
    prev = lib.io_get_winograd(), lib.io_get_bf16_p256()
    yield lib
    lib.io_set_winograd(prev[0])
    lib.io_set_bf16_p256(prev[1])


def _net(dtype, state):
    if ("net", dtype) not in _CACHE:
        _CACHE["net", dtype] = resnet_cls.ResNet(5, euo.HEADS, dtype=dtype).cuda()
    net = _CACHE["net", dtype]
    net.load_state_dict(euo.state_dict_of(state), strict=True)
    net.eval()
    return net


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _tapped(net, x8, N, H, W):
    """one io_net_forward_eval_taps call -> (tap buffer on the device, logits, routes)"""
    dev = x8.device
    ws = torch.empty(net.plan.workspace_bytes_hw(N, H, W), dtype=torch.uint8, device=dev)
    tdt = engine.TORCH_DTYPE[net.dtype]
    nb = net.plan.eval_taps_bytes(N, H, W)
    taps = torch.full((nb // tdt.itemsize,), float("nan"), dtype=tdt, device=dev)
    logits = torch.full((N, net.plan.num_logits), float("nan"), device=dev)
    routes = net.plan.forward_eval_taps(net.flat_params, net.flat_running, x8, N, H, W, ws, logits, taps, routes=True)
    torch.cuda.synchronize()
    return taps, logits, routes


def _units(net, taps, N, H, W, upto):
    offs = [net.plan.eval_tap_offset(N, H, W, k) for k in range(euo.NTAPS)]
    return euo.taps_to_units(taps.view(torch.uint8).cpu(), offs, net.dtype, N, H, W, upto)


def _hold(case, what, state, x, units, logits, ec):
    """every covered unit (and, where the case covers all, the logits) under its bar; -> (worst err / bar, unit, err, bar)"""
    dtype, upto = case[0], case[5]
    got = units + ([logits.double().cpu()] if upto is None else [])
    stored = units + [None] * (euo.NTAPS - len(units))
    ref = euo.reference(state, x, stored, len(got))
    err = euo.errors(got, ref)
    worst = sbo.worst_ratio(err, ec, lambda u: euo.floor_of(dtype, u))
    print("%s %s: worst error / bar %.3f (%s: %.2e / %.2e)" % (euo.case_id(case), what, worst[0], euo.UNIT_NAMES[worst[1]],
                                                                worst[2], worst[3]))
    bars = euo.bars(dtype, ec)
    bad = ["%s %.3e > %.3e" % (euo.UNIT_NAMES[u], err[u], bars[u]) for u in range(len(err)) if not err[u] < bars[u]]
    assert not bad, (euo.case_id(case), what, len(bad), bad[:24])
    return worst


@pytest.mark.parametrize("case", euo.CASES, ids=euo.case_id)
def test_every_eval_unit_against_the_fp64_oracle(case, switches):
    dtype, N, H, W, modes, upto = case
    lib = switches
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert cu == euo.NCU, "the launch predictions hold on %d CUs, this device has %d" % (euo.NCU, cu)
    state = euo.make_state(dtype, N, H, W)
    x5, x = euo.make_input(dtype, N, H, W)
    ec = euo.noise_floor(dtype, N, H, W, upto)[0]
    net = _net(dtype, state)
    x8 = engine.pack_nchw(x5.cuda(), dtype=dtype)
    assert tuple(x8.shape) == (N, H, W, 8) and float(x8[..., 5:].float().abs().max()) == 0.0
    ntap = euo.NTAPS if upto is None else upto

    lib.io_set_winograd(1)
    first = None
    for mode in (modes or (lib.io_get_bf16_p256(),)):
        lib.io_set_bf16_p256(mode)
        taps, logits, routes = _tapped(net, x8, N, H, W)
        assert not bool(torch.isnan(taps).any()) and not bool(torch.isnan(logits).any())
        assert routes == [p["route"] for p in euo.predict(dtype, N, H, W, mode)], (mode, routes)
        units = _units(net, taps, N, H, W, ntap)
        _hold(case, "p256 mode %d" % mode if modes else "winograd on", state, x, units, logits, ec)
        if first is None:
            first = (taps, logits, units)
            # the same call again, and the product entry point on the same inputs: the same bits
            taps2, logits2, _ = _tapped(net, x8, N, H, W)
            assert torch.equal(_bits(taps2), _bits(taps)) and torch.equal(_bits(logits2), _bits(logits))
            with torch.no_grad():
                plain = net.forward_packed(x8, 1)
            torch.cuda.synchronize()
            assert torch.equal(_bits(plain), _bits(logits))

    if dtype == "fp32":
        lib.io_set_winograd(0)
        taps, logits, routes = _tapped(net, x8, N, H, W)
        assert not bool(torch.isnan(taps).any()) and not bool(torch.isnan(logits).any())
        assert routes == [0] * 53
        units = _units(net, taps, N, H, W, ntap)
        _hold(case, "winograd off", state, x, units, logits, ec)
        wino = euo.wino_units(dtype, N, H, W)
        assert wino and euo.UNIT_NAMES[wino[0]].endswith(".a2") and wino[0] < ntap
        for i in range(wino[0]):
            assert torch.equal(units[i], first[2][i]), euo.UNIT_NAMES[i]
        assert not torch.equal(units[wino[0]], first[2][wino[0]]), \
            "%s is bit-identical with Winograd on and off: the form did not run" % euo.UNIT_NAMES[wino[0]]


def test_rejects_short_buffers():
    """short tap buffer / short route array: refused before anything is launched (the NaN fill survives)"""
    net = engine.Net(5, euo.HEADS)
    N, H, W = 1, 32, 64
    dev = torch.device("cuda:0")
    params = torch.zeros(net.param_floats, device=dev)
    running = torch.ones(net.running_floats, device=dev)
    x8 = torch.zeros(N, H, W, 8, device=dev)
    ws = torch.empty(net.workspace_bytes_hw(N, H, W), dtype=torch.uint8, device=dev)
    logits = torch.full((N, net.num_logits), float("nan"), device=dev)
    taps = torch.full((net.eval_taps_bytes(N, H, W) // 4,), float("nan"), device=dev)
    with pytest.raises(RuntimeError):
        net.forward_eval_taps(params, running, x8, N, H, W, ws, logits, taps[:-1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(logits).all()) and bool(torch.isnan(taps).all())
    assert net.forward_eval_taps(params, running, x8, N, H, W, ws, logits, None) is None      # taps are optional
    torch.cuda.synchronize()
    assert not bool(torch.isnan(logits).any()) and bool(torch.isnan(taps).all())


# ---- the driver on an H x W input in bf16 ------------------------------------------------------------------------------------
BF16_LOGITS_BAR = 1e-2         # tests/test_gpu_bf16.py: bf16 eval-mode logits against the oracle, on the damped network it uses


def test_orig_mode_driver_in_bf16():
    import instaorder_amd as ia
    from instaorder_amd import inference
    algo = "InstaOrderNet_o"
    sd = synthetic.make_state_dict(97, 5, 2, prefix="module.", style="kaiming")
    for k in sd:                 # (the damped residual branches of tests/test_gpu_bf16.py: end-to-end bf16 parity needs them)
        if k.endswith("bn3.weight"):
            sd[k] = (sd[k] * 0.1).astype(np.float32)
    rs = np.random.RandomState(5)
    for k in sd:                 # running estimates away from 0 / 1
        if k.endswith("running_mean"):
            sd[k] = (0.1 * rs.standard_normal(sd[k].shape)).astype(np.float32)
        elif k.endswith("running_var"):
            sd[k] = rs.uniform(0.5, 1.5, sd[k].shape).astype(np.float32)
    models = {}
    for dt in ("fp32", "bf16"):
        cfg = dict(algo=algo, lr=1e-3, weight_decay=1e-4, optim="SGD", backbone_arch="resnet50_cls", dtype=dt,
                   backbone_param=dict(in_channels=5, num_classes=2), use_rgb=True)
        m = ia.InstaOrderNet_o(cfg, dist_model=False)
        m.model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        m.switch_to("eval")
        assert m.net.dtype == dt
        models[dt] = m
    sc = synthetic.SyntheticReader(9, n_images=4, n_inst=4, empty_every=0).scenes[3]           # 131 x 102 -> 128 x 96
    rgb, masks = inference.orig_mode_inputs("cuda:0", sc["image"], sc["modal"])
    assert tuple(rgb.shape[-2:]) == (128, 96)
    res = {dt: inference.infer_order_batched(models[dt], rgb, masks, algo, return_logits=True) for dt in models}
    # fp64 oracle on the driver's own planes, unrounded (as tests/test_gpu_bf16.py holds bf16 logits to the oracle)
    state = sbo.state64(sd, prefix="module.")
    pairs = inference.upper_pairs(masks.shape[0])
    mk, img = masks.cpu().double(), rgb.cpu().double().expand(len(pairs), -1, -1, -1)
    mi, mj = mk[[a for a, _ in pairs]][:, None], mk[[b for _, b in pairs]][:, None]
    refs = []
    for xin in (torch.cat([mi, mj, img], 1), torch.cat([mj, mi, img], 1)):
        acts = []
        for i, u in enumerate(euo.UNITS):
            src = xin if u.get("src", 0) < 0 else acts[u["src"]]
            idt = acts[u["idt"]] if u.get("idt") is not None else None
            if u["kind"] == "head":
                feat = torch.flatten(src.mean(dim=(2, 3)), 1)
                acts.append(torch.nn.functional.linear(feat, state["fc.weight"], state["fc.bias"]))
            else:
                acts.append(euo.exact_unit(state, i, src, idt))
        refs.append(acts[-1])
    ref = torch.cat(refs, 1)
    got = torch.from_numpy(res["bf16"]["pair_logits"]).double()
    e = sbo.err_max(got, ref)
    e32 = sbo.err_max(torch.from_numpy(res["fp32"]["pair_logits"]).double(), ref)
    print("orig mode 128 x 96: bf16 logits rel err vs fp64 oracle %.3e (fp32 run: %.3e)" % (e, e32))
    assert e < BF16_LOGITS_BAR
    # a logit moves by at most delta = bar * max|ref|, a sigmoid by a quarter of that, and so does the mean of two
    delta = BF16_LOGITS_BAR * float(ref.abs().max()) / 4
    margin = inference.decision_margins(torch.from_numpy(res["fp32"]["pair_logits"]), algo)["occ"]
    decided = 0
    for k, (i, j) in enumerate(pairs):
        for col, (a, b) in enumerate(((i, j), (j, i))):
            if margin[k, col] > delta:
                decided += 1
                assert res["bf16"]["occ_order"][a, b] == res["fp32"]["occ_order"][a, b], (i, j, col, margin[k, col])
    print("orig mode 128 x 96: %d of %d decisions lie outside the bf16 bar and agree" % (decided, 2 * len(pairs)))
    assert decided > 0
