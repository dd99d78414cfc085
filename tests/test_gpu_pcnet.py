"""PCNet-M order recovery on the GPU: the kernels of csrc/unet.hip against torch in fp64, the UNet forward of
instaorder_amd/unet.py against the restatement (tests/pcnet_ref.py) on both routes of the 32-channel layers, the head,
``inference.infer_order`` against the run of the real reference in tests/golden/pcnet.npz and against the restatement,
``evaluate.evaluate(order_method='PartialCompletionMask')`` and ``PartialCompletionMask.forward_only``.

Bars.  Single launches: max|got - ref| / max|ref| < 2e-5 (the project's).  The whole forward: at most
max(3 x e32, 2e-5), e32 = the error of the same network run by torch in fp32 on the CPU against fp64 (the factor-3 anchor
rule of helpers.check_against_anchor; the floor is the single-launch bar).  Thresholded outputs: every pixel that is not
*undecided* (pcnet_ref: within 2 x bar x max|logits| of the threshold in fp64) must match and a count may differ by at most
its patch's undecided pixels; the fixture conditions (tests/test_pcnet_cpu.py) keep an order from flipping inside that.
Kernel outputs sit in guarded allocations prefilled with NaN; the error paths are argument checks that return before any
launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcnet_ref as pr
from helpers import load_golden, rel_err
from instaorder_amd import _lib, evaluate, inference, poly, rle, unet
from test_gpu_conv_edges import Guarded
from test_gpu_ops import L, P, ST

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = pr.BAR
CFG = dict(algo="PartialCompletionMask", backbone_arch="unet025", backbone_param=dict(in_channels=2, n_classes=2),
           use_rgb=False, inmask_weight=5.0, optim="SGD", lr=1e-3, weight_decay=1e-4)


@pytest.fixture(autouse=True)
def _route():
    prev = L().io_get_unet_co32()
    L().io_set_unet_co32(1)
    yield
    L().io_set_unet_co32(prev)


@pytest.fixture(scope="module")
def g():
    return load_golden("pcnet")


@pytest.fixture(scope="module")
def gsd(g):
    return {str(k): torch.from_numpy(g["sd/" + str(k)]) for k in g["key_order"]}


def golden_scene(g, tag):
    return g[tag + "/inmodal"], g[tag + "/category"], g[tag + "/bboxes"], int(g[tag + "/input_size"])


def model_with(sd, arch="unet025"):
    import instaorder_amd as ia
    m = ia.PartialCompletionMask(dict(CFG, backbone_arch=arch))
    m.model.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)
    m.switch_to("eval")
    return m


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().to(DEV)


# ---- io_conv3x3_co32_fwd --------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 16, 16), (3, 32, 32), (2, 16, 48), (1, 40, 24)]
CONV_CASES = [(ci, s) for ci in (8, 32, 64, 128) for s in SHAPES] + [(64, (1, 256, 256))]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("ci,shape", CONV_CASES, ids=["ci%d-%dx%dx%d" % ((c,) + s) for c, s in CONV_CASES])
def test_conv3x3_co32(ci, shape, relu):
    N, H, W = shape
    gen = torch.Generator().manual_seed(ci * 1000 + H * 10 + W)
    real = 2 if ci == 8 else ci
    x = torch.zeros(N, ci, H, W, dtype=torch.float64)
    x[:, :real] = torch.randn(N, real, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(32, ci, 3, 3, generator=gen, dtype=torch.float64) / np.sqrt(9 * real)
    b = torch.randn(32, generator=gen, dtype=torch.float64)            # both signs: ReLU cuts about half
    x, w, b = x.float().double(), w.float().double(), b.float().double()
    ref = F.conv2d(x[:, :real], w[:, :real], b, padding=1)
    if relu:
        assert 0.25 < float((ref < 0).double().mean()) < 0.75
        ref = F.relu(ref)
    wp = w.permute(2, 3, 1, 0).reshape(9, ci, 32).contiguous().float().to(DEV)
    y = Guarded((N, H, W, 32), torch.float32)
    _lib.check(L().io_conv3x3_co32_fwd(P(nhwc(x)), P(wp), P(b.float().to(DEV)), y.p(), N, H, W, ci, 32, relu, ST()), "co32")
    assert y.intact()
    got = y.t.permute(0, 3, 1, 2).double().cpu()
    assert not torch.isnan(got).any(), "unwritten outputs"
    e = rel_err(got.numpy(), ref.numpy())
    print("DIST conv3x3_co32 ci=%d %s relu=%d: %.3e" % (ci, shape, relu, e))
    assert e < BAR


def test_conv3x3_co32_refuses_without_writing():
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    w, b = torch.zeros(9 * 128 * 32, device=DEV), torch.zeros(64, device=DEV)
    y = Guarded((1, 4, 4, 64), torch.float32)
    for args in ((1, 4, 4, 64, 64), (1, 4, 4, 16, 32), (1, 4, 4, 96, 32), (0, 4, 4, 32, 32), (1, 0, 4, 32, 32)):
        rc = L().io_conv3x3_co32_fwd(P(x), P(w), P(b), y.p(), *args, 1, ST())
        assert rc != 0 and len(_lib.last_error()) > 0, args
    assert L().io_conv3x3_co32_fwd(P(x), P(w), None, y.p(), 1, 4, 4, 32, 32, 1, ST()) != 0
    assert y.untouched()


# ---- io_maxpool2x2_fwd / io_up2x_concat_fwd ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 16, 16, 32), (1, 2, 2, 64)])
def test_maxpool2x2(shape):
    N, H, W, Cc = shape
    x = torch.randn(N, Cc, H, W, generator=torch.Generator().manual_seed(H))
    out = Guarded((N, H // 2, W // 2, Cc), torch.float32)
    _lib.check(L().io_maxpool2x2_fwd(P(nhwc(x)), N, H, W, Cc, out.p(), ST()), "pool")
    assert out.intact()
    assert torch.equal(out.t.permute(0, 3, 1, 2).cpu(), F.max_pool2d(x, 2))


def test_maxpool2x2_refuses_odd_sizes():
    x = torch.zeros(1, 5, 4, 32, device=DEV)
    out = Guarded((1, 2, 2, 32), torch.float32)
    for h, w, c in ((5, 4, 32), (4, 3, 32)):
        assert L().io_maxpool2x2_fwd(P(x), 1, h, w, c, out.p(), ST()) != 0 and "must be even" in _lib.last_error()
    assert L().io_maxpool2x2_fwd(P(x), 1, 4, 4, 6, out.p(), ST()) != 0 and len(_lib.last_error()) > 0
    assert out.untouched()


@pytest.mark.parametrize("N,h,w", [(2, 4, 4), (1, 1, 1)])
def test_up2x_concat(N, h, w):
    C1 = C2 = 32
    gen = torch.Generator().manual_seed(h + 3)
    x1 = torch.randn(N, C1, h, w, generator=gen, dtype=torch.float64).float()
    x2 = torch.randn(N, C2, 2 * h, 2 * w, generator=gen, dtype=torch.float64).float()
    out = Guarded((N, 2 * h, 2 * w, C2 + C1), torch.float32)
    _lib.check(L().io_up2x_concat_fwd(P(nhwc(x2)), P(nhwc(x1)), N, h, w, C2, C1, out.p(), ST()), "up2x_concat")
    assert out.intact()
    got = out.t.permute(0, 3, 1, 2).cpu()
    assert torch.equal(got[:, :C2], x2), "the skip half is a copy"
    ref = F.interpolate(x1.double(), scale_factor=2, mode="bilinear", align_corners=True)
    assert rel_err(got[:, C2:].double().numpy(), ref.numpy()) < 1e-6          # the bar of test_upsample2x_bilinear
    assert L().io_up2x_concat_fwd(P(nhwc(x2)), P(nhwc(x1)), N, h, w, 30, C1, out.p(), ST()) != 0


# ---- the UNet forward ---------------------------------------------------------------------------------------------------
def scene_inputs(g, tag, take=(0, 7, 12)):
    inmodal, category, bboxes, size = golden_scene(g, tag)
    ind = pr.pair_index(inmodal, "all")[list(take)]
    tp, ep = pr.patches(inmodal, bboxes, ind, size)
    return torch.from_numpy(np.stack([tp, ep], 1).astype(np.float32))


_FWD = {}


def forward_case(g, gsd, arch, size):
    """(x, fp64 logits, e32, the net on the GPU), computed once per case"""
    key = (arch, size)
    if key not in _FWD:
        sd = gsd if arch == "unet025" else pr.seeded_state(arch, 7)
        x = scene_inputs(g, "s32" if size == 32 else "s64")
        with torch.no_grad():
            ref = pr.unet_forward(sd, x.double())
            e32 = rel_err(pr.unet_forward(sd, x).numpy(), ref.numpy())
        net = getattr(unet, arch)(2)
        net.load_state_dict(sd, strict=True)
        _FWD[key] = (x, ref, e32, net.to(DEV).eval())
    return _FWD[key]


FWD_CASES = [("unet025", 32), ("unet1", 32), ("unet2", 32), ("unet2", 64)]


@pytest.mark.parametrize("arch,size", FWD_CASES)
def test_unet_forward_against_fp64(g, gsd, arch, size):
    x, ref, e32, net = forward_case(g, gsd, arch, size)
    with torch.no_grad():
        got = net(x.to(DEV)).double().cpu()
    e = rel_err(got.numpy(), ref.numpy())
    bound = max(3 * e32, BAR)
    print("DIST unet forward %s %d: %.3e (torch fp32 on the CPU %.3e, bound %.3e)" % (arch, size, e, e32, bound))
    assert got.shape == ref.shape and e <= bound
    if arch == "unet025":          # the reference's own fp32 logits of the same three patches
        assert rel_err(got.numpy(), g["fo_logits"].astype(np.float64)) <= bound + e32


@pytest.mark.parametrize("arch,size", FWD_CASES)
def test_routes_agree(g, gsd, arch, size):
    """the 32-channel layers through io_conv2d_fwd_bias_dt with Cout padded to 64 give the same logits"""
    x, ref, e32, net = forward_case(g, gsd, arch, size)
    with torch.no_grad():
        on = net(x.to(DEV)).double().cpu()
        assert unet.set_co32(False) is True
        off = net(x.to(DEV)).double().cpu()
    assert any(l[4] for l in net.operands(True)[0]) and not any(l[4] for l in net.operands(False)[0])
    e = rel_err(off.numpy(), on.numpy())
    print("DIST unet routes %s %d: %.3e; padded route against fp64 %.3e" % (arch, size, e, rel_err(off.numpy(), ref.numpy())))
    assert e <= 2 * BAR
    assert rel_err(off.numpy(), ref.numpy()) <= max(3 * e32, BAR)


# ---- io_unet_head -------------------------------------------------------------------------------------------------------
def test_head_kernel_alone():
    Pn, HW, Cs = 3, 40 * 24, 32
    gen = torch.Generator().manual_seed(9)
    act = torch.randn(Pn, HW, Cs, generator=gen)
    wo, bo = torch.randn(2, Cs, generator=gen) / 4, torch.randn(2, generator=gen) / 4
    m2 = (torch.rand(Pn, HW, generator=gen) < 0.4).float()
    m2[0, :7] = 2.0                                                    # a value that is neither 0 nor 1
    m1 = (torch.rand(Pn, HW, generator=gen) < 0.5).float()
    tgt = (torch.rand(Pn, HW, generator=gen) < 0.5).to(torch.uint8)
    th = 0.6
    l = act.double() @ wo.double().t() + bo.double()
    d = (l[..., 1] - l[..., 0]) - pr.logit_threshold(th)
    sure = d.abs() > 2 * BAR * float(l.abs().max())
    vis = torch.where(m2 == 1, torch.zeros_like(m1), m1)
    vote = ((d > 0).float() > vis) & (m2 == 1)
    ce = F.cross_entropy(l.view(-1, 2), tgt.view(-1).long(), reduction="none").view(Pn, HW)
    want = [float(ce[m2 != 0].sum()), float(ce[m2 == 0].sum())]
    nf = L().io_unet_head_partial_floats(Pn, HW)
    outs = []
    for _ in range(2):
        comp, counts = Guarded((Pn, HW), torch.uint8, fill=255), Guarded((Pn,), torch.int32, fill=-1)
        logits, part, sums = Guarded((Pn, HW, 2), torch.float32), Guarded((nf,), torch.float32), Guarded((2,), torch.float32)
        _lib.check(L().io_unet_head(P(act.to(DEV)), P(wo.to(DEV)), P(bo.to(DEV)), P(m1.to(DEV)), P(m2.to(DEV)), P(tgt.to(DEV)),
                                    Pn, HW, Cs, th, comp.p(), counts.p(), logits.p(), part.p(), nf, sums.p(), ST()), "head")
        assert all(o.intact() for o in (comp, counts, logits, part, sums))
        outs.append((comp.t.cpu(), counts.t.cpu(), logits.t.cpu(), sums.t.cpu()))
    comp, counts, logits, sums = outs[0]
    assert rel_err(logits.double().numpy(), l.numpy()) < BAR
    assert torch.equal(comp.bool()[sure], (d > 0)[sure])
    slack = (~sure & (m2 == 1)).sum(1)
    assert ((counts.long() - vote.sum(1)).abs() <= slack).all()
    assert torch.equal(counts.long(), ((comp.float() > vis) & (m2 == 1)).sum(1)), "the count is the sum of its own votes"
    for k in range(2):
        assert abs(float(sums[k]) - want[k]) <= 1e-5 * abs(want[k])
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "two runs differ"
    # refused: a threshold outside (0, 1), a short partials buffer, half of the loss arguments
    comp = Guarded((Pn, HW), torch.uint8, fill=255)
    args = (P(act.to(DEV)), P(wo.to(DEV)), P(bo.to(DEV)), P(m1.to(DEV)), P(m2.to(DEV)))
    assert L().io_unet_head(*args, None, Pn, HW, Cs, 1.0, comp.p(), None, None, None, 0, None, ST()) != 0
    part = torch.zeros(nf, device=DEV)
    assert L().io_unet_head(*args, P(tgt.to(DEV)), Pn, HW, Cs, 0.5, comp.p(), None, None, P(part), nf - 1, P(part), ST()) != 0
    assert L().io_unet_head(*args, P(tgt.to(DEV)), Pn, HW, Cs, 0.5, comp.p(), None, None, None, 0, None, ST()) != 0
    assert comp.untouched()


def check_against_restatement(r, occ, pats, label):
    """completions, counts and occ values of the device against the restatement, up to the undecided pixels"""
    tp, ep, comp = (np.stack(p) for p in pats)
    assert np.array_equal(tp, r["target"]) and np.array_equal(ep, r["eraser"]), label
    assert not ((comp != r["comp"]) & ~r["undecided_map"] & (ep == 1)).any(), label
    d = (r["logits"][:, 1] - r["logits"][:, 0]).numpy() - pr.logit_threshold(0.5)
    und_all = np.abs(d) <= 2 * BAR * float(r["logits"].abs().max())
    assert not ((comp != r["comp"]) & ~und_all).any(), label
    slack = np.zeros(occ.shape)
    for k, (t, e) in enumerate(r["ind"]):
        slack[t, e] = r["undecided"][k] * r["ratio2"][k]
    assert occ.dtype == np.float32 and (np.abs(occ.astype(np.float64) - r["occ_value"]) <= slack + 1e-6).all(), label
    print("UNDECIDED %s: %d of %d eraser pixels; completions that differ: %d" % (label, int(r["undecided"].sum()),
                                                                               int((ep == 1).sum()), int((comp != r["comp"]).sum())))


# ---- infer_order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["s32", "s64"])
def test_infer_order_golden_scenes(g, gsd, tag):
    inmodal, category, bboxes, size = golden_scene(g, tag)
    m = model_with(gsd)
    out = inference.infer_order(m, None, inmodal, category, bboxes, "all", th=0.5, input_size=size, min_input_size=16,
                                debug_info=True)
    order, ind, tp, ep, ap = out
    assert np.array_equal(ind, g[tag + "/ind"]) and order.dtype == np.int64
    assert all(p.dtype == np.uint8 for p in tp + ep + ap)
    assert np.array_equal(np.stack(tp), g[tag + "/target"]) and np.array_equal(np.stack(ep), g[tag + "/eraser"])
    r = pr.infer_order(gsd, inmodal, category, bboxes, "all", 0.5, size)
    occ, _, pats = inference.infer_occ_values(m, inmodal, category, bboxes, "all", 0.5, size, keep_patches=True)
    check_against_restatement(r, occ, pats, tag)
    # the reference's own run: its order matrix exactly, its occ values and completions up to the undecided pixels
    assert np.array_equal(order, g[tag + "/order"])
    slack = np.zeros(occ.shape)
    for k, (t, e) in enumerate(r["ind"]):
        slack[t, e] = r["undecided"][k] * r["ratio2"][k]
    assert (np.abs(occ.astype(np.float64) - g[tag + "/occ_value"]) <= slack + 1e-6).all()
    assert not ((np.stack(ap) != g[tag + "/comp"]) & ~r["undecided_map"] & (np.stack(ep) == 1)).any()
    assert np.array_equal(inference.infer_order(m, None, inmodal, category, bboxes, "all", input_size=size), order)


@pytest.fixture(scope="module")
def rest():
    sd = pr.restatement_state()
    return sd, model_with(sd), pr.restatement_scenes()


@pytest.mark.parametrize("tag", ["larger", "smaller", "outside", "nbor"])
def test_infer_order_restatement_scenes(rest, tag):
    sd, m, scenes = rest
    inmodal, category, bboxes, size, pairs = scenes[tag]
    r = pr.infer_order(sd, inmodal, category, bboxes, pairs, 0.5, size)
    for rules in ("host", "device"):
        occ, ind, pats = inference.infer_occ_values(m, inmodal, category, bboxes, pairs, 0.5, size, keep_patches=True,
                                                    mask_rules=rules)
        assert np.array_equal(ind, r["ind"]), (tag, rules)
        check_against_restatement(r, occ, pats, tag)
        order = inference.infer_order(m, None, inmodal, category, bboxes, pairs, input_size=size, mask_rules=rules)
        assert np.array_equal(order, r["order"]), (tag, rules)


def test_infer_order_single_instance_launches_nothing(rest):
    sd, m, scenes = rest
    inmodal, category, bboxes, size, pairs = scenes["single"]
    calls = []
    real = m.net.run
    m.net.run = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        out = inference.infer_order(m, None, inmodal, category, bboxes, pairs, input_size=size, debug_info=True)
    finally:
        del m.net.run
    assert isinstance(out, np.ndarray) and out.shape == (1, 1) and not out.any() and not calls


def test_infer_order_encoded_masks_and_chunks(rest):
    sd, m, scenes = rest
    H, W = 72, 96
    rs = np.random.RandomState(4)
    segs = []
    for i in range(4):
        cx, cy, a, b = rs.uniform(30, 66), rs.uniform(24, 48), rs.uniform(12, 22), rs.uniform(10, 18)
        t = np.sort(rs.uniform(0, 2 * np.pi, 9))
        segs.append([np.round(np.stack([cx + a * np.cos(t), cy + b * np.sin(t)], 1), 2).reshape(-1).tolist()])
    pm = poly.PolyMasks(segs, H, W)
    dense = pm.to_dense()
    rm = rle.RLEMasks.from_dense(dense)
    category = np.ones(4, np.int64)
    bboxes = evaluate.expand_bbox([[int(min(s[0][0::2])), int(min(s[0][1::2])), int(max(s[0][0::2]) - min(s[0][0::2])) + 1,
                                    int(max(s[0][1::2]) - min(s[0][1::2])) + 1] for s in segs], 3.0)
    r = pr.infer_order(sd, dense, category, bboxes, "all", 0.5, 32)
    base = None
    for name, masks, mp in (("dense", dense, 64), ("rle", rm, 64), ("poly", pm, 64), ("dense", dense, 1), ("dense", dense, 7),
                            ("rle", rm, 7)):
        occ, ind, pats = inference.infer_occ_values(m, masks, category, bboxes, "all", 0.5, 32, keep_patches=True,
                                                    max_pairs=mp, mask_rules="device" if name != "dense" else "host")
        got = (occ, ind) + tuple(np.stack(p) for p in pats)
        if base is None:
            base = got
            check_against_restatement(r, occ, pats, "encoded")
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), (name, mp)


# ---- evaluate / forward_only --------------------------------------------------------------------------------------------
class _Reader(object):
    """three synthetic images in the InstaOrder reader's form, with seeded ground-truth occlusion matrices"""

    def __init__(self):
        self.scenes = []
        for k, (n, H, W, side) in enumerate([(3, 90, 120, 40), (3, 128, 100, 52), (2, 70, 70, 30)]):
            m, c, _ = pr.scene(60 + k, n, H, W, side)
            bb = []
            for mask in m:
                ys, xs = np.where(mask > 0)
                bb.append([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1])
            gt = (np.random.RandomState(70 + k).rand(n, n) < 0.5).astype(np.int64)
            np.fill_diagonal(gt, 0)
            self.scenes.append((m, c, np.array(bb), gt))

    def get_image_length(self):
        return len(self.scenes)

    def get_image_instances(self, i, with_gt=False):
        m, c, bb, _ = self.scenes[i]
        return m, c, bb, None, "scene%d" % i

    def get_gt_ordering(self, i, kind="occlusion", rm_bidirec=0):
        return self.scenes[i][3].copy()


def test_evaluate_partial_completion_mask():
    """tools/test.py:435-439 through evaluate.evaluate: P / R / F1 of the restatement's matrices.  (Before this branch
    existed the call raised 'No such order method: PartialCompletionMask'.)"""
    rd = _Reader()
    cfg = dict(trainval_dataset="PartialCompDataset", dataset="InstaOrder", patch_or_image="patch", input_size=256,
               enlarge_box=3.0, remove_occ_bidirec=0, use_category=False)
    boxes = [evaluate.expand_bbox(s[2], 3.0) for s in rd.scenes]
    sd = pr.calibrate_outc_bias(pr.seeded_state("unet025", 51), [(s[0], s[1], b, 256) for s, b in zip(rd.scenes, boxes)])
    rows = []
    for s, b in zip(rd.scenes, boxes):
        r = pr.infer_order(sd, s[0], s[1], b, "all", 0.5, 256)
        slack = np.zeros(r["occ_value"].shape)
        for k, (t, e) in enumerate(r["ind"]):
            slack[t, e] = r["undecided"][k] * r["ratio2"][k]
        gap = np.abs(r["occ_value"].astype(np.float64) - r["occ_value"].T)
        assert ((gap > slack + slack.T) | ((gap == 0) & (slack + slack.T == 0))).all(), "a pair the undecided pixels could flip"
        rows.append(inference.eval_order_recall_precision_f1(r["order"], s[3], 0))
    want = np.mean(np.asarray(rows, np.float64), 0)
    m = model_with(sd)

    def no_image(fn):
        raise AssertionError("PCNet-M reads no picture")

    res = evaluate.evaluate(m, rd, no_image, cfg, "PartialCompletionMask", pairs="all", order_th=0.5, return_orders=True)
    got = [res["recall"], res["precision"], res["f1"]]
    print("EVALUATE PartialCompletionMask: recall %.3f precision %.3f f1 %.3f (restatement %s)" % (tuple(got) + (want,)))
    assert np.allclose(got, want, rtol=0, atol=1e-9) and res["num_test_images"] == 3
    assert sum(int(o[0].sum()) for o in res["orders"].values()) > 0


def test_forward_only_against_the_reference(g, gsd):
    m = model_with(gsd)
    m.set_input(rgb=None, mask=torch.from_numpy(g["fo_mask"]), eraser=torch.from_numpy(g["fo_eraser"]),
                target=torch.from_numpy(g["fo_target"]))
    ret, loss = m.forward_only(ret_loss=True)
    ret2, loss2 = m.forward_only(ret_loss=True)
    assert ret["common_tensors"] == [] and len(ret["mask_tensors"]) == 4
    got = float(loss["loss"])
    print("LOSS forward_only %.8f, reference %.8f (fp64 %.8f)" % (got, float(g["fo_loss"]), float(g["fo_loss64"])))
    assert abs(got - float(g["fo_loss64"])) <= 1e-5 * abs(float(g["fo_loss64"]))
    assert abs(got - float(g["fo_loss"])) <= 1e-5 * abs(float(g["fo_loss"]))
    assert torch.equal(loss["loss"], loss2["loss"]), "two runs of the loss differ"
    x = torch.from_numpy(np.concatenate([g["fo_mask"], g["fo_eraser"]], 1)).double()
    with torch.no_grad():
        l64 = pr.unet_forward(gsd, x)
    sure = ((l64[:, 1] - l64[:, 0]).abs() > 2 * BAR * float(l64.abs().max())).unsqueeze(1)
    comp = ret["mask_tensors"][2].cpu()
    assert comp.shape == g["fo_comp"].shape and torch.equal(comp[sure], torch.from_numpy(g["fo_comp"])[sure])
    assert torch.equal(ret["mask_tensors"][1].cpu(), torch.from_numpy(g["fo_vis_combo"]))
    assert torch.equal(ret["mask_tensors"][3], torch.from_numpy(g["fo_vis_target"]))
    assert m.forward_only(ret_loss=False)["mask_tensors"][2].shape == comp.shape
