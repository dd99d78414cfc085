"""PCNet-M order recovery, the parts that need no GPU: the restatement (tests/pcnet_ref.py) against the run of the real
reference stored in tests/golden/pcnet.npz, the state-dict surface of instaorder_amd.unet, the BatchNorm fold and the
padded / concatenated filter layout (the packed operands run through F.conv2d on the stored layouts), the order rule,
the refused arguments, and the conditions the fixtures must keep meeting.

What is pinned to what: the golden scenes have boxes of side exactly input_size, so the reference ran them with an
identity resize; every other resize is held to the restatement only (no cv2 where the golden is made)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcnet_ref as pr
from helpers import load_golden, rel_err
from instaorder_amd import inference, unet

CFG = dict(algo="PartialCompletionMask", backbone_arch="unet025", backbone_param=dict(in_channels=2, n_classes=2),
           use_rgb=False, inmask_weight=5.0, optim="SGD", lr=1e-3, weight_decay=1e-4)


@pytest.fixture(scope="module")
def g():
    return load_golden("pcnet")


@pytest.fixture(scope="module")
def gsd(g):
    return {str(k): torch.from_numpy(g["sd/" + str(k)]) for k in g["key_order"]}


def golden_scene(g, tag):
    return g[tag + "/inmodal"], g[tag + "/category"], g[tag + "/bboxes"], int(g[tag + "/input_size"])


# ---- the restatement against the reference ---------------------------------------------------------------------------
def test_restatement_logits_and_loss_match_the_reference(g, gsd):
    x = torch.from_numpy(np.concatenate([g["fo_mask"], g["fo_eraser"]], 1))
    with torch.no_grad():
        l64 = pr.unet_forward(gsd, x.double())
        l32 = pr.unet_forward(gsd, x)
    # fp64 against the reference's own modules run in fp64: 1e-12
    assert rel_err(l64.numpy(), g["fo_logits64"]) < 1e-12
    tgt, er = torch.from_numpy(g["fo_target"]), torch.from_numpy(g["fo_eraser"][:, 0])
    w = float(g["inmask_weight"])
    loss64 = float(pr.masked_loss(l64, tgt, er, w))
    assert abs(loss64 - float(g["fo_loss64"])) <= 1e-12 * abs(float(g["fo_loss64"]))
    # in the reference's dtype: its fp32 logits, loss and comp exactly
    assert np.array_equal(l32.numpy(), g["fo_logits"])
    loss32 = pr.masked_loss_as_reference(l32, tgt, er, w)
    assert loss32.dtype == torch.float32 and np.float32(loss32.item()) == g["fo_loss"]
    comp = l32.argmax(1, keepdim=True).float()
    mask, era = torch.from_numpy(g["fo_mask"]), torch.from_numpy(g["fo_eraser"])
    comp[era == 0] = (mask > 0).float()[era == 0]
    assert np.array_equal(comp.numpy(), g["fo_comp"])


@pytest.mark.parametrize("tag", ["s32", "s64"])
def test_restatement_infer_order_matches_the_reference(g, gsd, tag):
    """in the reference's arithmetic (fp32, one patch per forward, softmax > th) every output is the reference's, bit for
    bit; the fp64 anchor differs from it only at undecided pixels"""
    inmodal, category, bboxes, size = golden_scene(g, tag)
    r = pr.infer_order(gsd, inmodal, category, bboxes, "all", 0.5, size, as_reference=True)
    assert np.array_equal(r["ind"], g[tag + "/ind"])
    assert np.array_equal(r["target"], g[tag + "/target"]) and np.array_equal(r["eraser"], g[tag + "/eraser"])
    assert np.array_equal(r["comp"], g[tag + "/comp"])
    assert np.array_equal(r["occ_value"], g[tag + "/occ_value"])
    assert np.array_equal(r["order"], g[tag + "/order"])
    assert r["order"].dtype == g[tag + "/order"].dtype and r["occ_value"].dtype == g[tag + "/occ_value"].dtype
    a = pr.infer_order(gsd, inmodal, category, bboxes, "all", 0.5, size)
    differ = a["comp"] != g[tag + "/comp"]
    print("ANCHOR %s: fp64 completions differing from the reference's: %d (undecided under the erasers: %d)"
          % (tag, int(differ.sum()), int(a["undecided"].sum())))
    d = (a["logits"][:, 1] - a["logits"][:, 0]).numpy() - pr.logit_threshold(0.5)
    assert not (differ & (np.abs(d) > 2 * pr.BAR * float(a["logits"].abs().max()))).any()
    assert np.array_equal(a["order"], g[tag + "/order"])


# ---- the fixtures stay meaningful ------------------------------------------------------------------------------------
def _conditions(r, label):
    share, und, ok = pr.fixture_conditions(r)
    print("FIXTURE %s: completed share %.3f, undecided share %.5f, decisive pair %s" % (label, share, und, ok))
    assert 0.2 <= share <= 0.8, (label, share)
    assert und <= 0.01, (label, und)
    assert ok, label


@pytest.mark.parametrize("tag", ["s32", "s64"])
def test_fixture_conditions_golden(g, gsd, tag):
    inmodal, category, bboxes, size = golden_scene(g, tag)
    _conditions(pr.infer_order(gsd, inmodal, category, bboxes, "all", 0.5, size), tag)


def test_fixture_conditions_restatement_scenes():
    sd = pr.restatement_state()
    for tag, (m, c, b, size, pairs) in pr.restatement_scenes().items():
        r = pr.infer_order(sd, m, c, b, pairs, 0.5, size)
        if tag == "single":
            assert len(r["ind"]) == 0 and not r["order"].any()
            continue
        _conditions(r, tag)
    nb = pr.restatement_scenes()["nbor"]
    ind = pr.pair_index(nb[0], "nbor")
    assert len(ind) and 4 not in ind, "the isolated instance must have no neighbour"
    out = pr.restatement_scenes()["outside"]
    r = pr.infer_order(sd, *out[:3], "all", 0.5, 32)
    assert all(r["eraser"][k].sum() == 0 and r["target"][k].sum() == 0 for k, (t, e) in enumerate(r["ind"]) if t == 4)


# ---- the module surface ----------------------------------------------------------------------------------------------
def key_list(sd):
    return sorted("%s %s %s" % (k, ",".join(str(d) for d in v.shape), str(v.dtype).replace("torch.", ""))
                  for k, v in sd.items())


@pytest.mark.parametrize("arch", ["unet025", "unet2"])
def test_state_dict_keys_shapes_dtypes(g, arch):
    from instaorder_amd import common_utils
    net = common_utils.FixModule(getattr(unet, arch)(2, n_classes=2))
    want = [str(k) for k in g["keys_" + arch]]
    if arch == "unet2":
        want = sorted("module." + k for k in want)
    assert key_list(net.state_dict()) == want
    assert list(pr.state_shapes(arch)) == [k[len("module."):] for k in net.state_dict()]


def test_reference_layout_checkpoint_loads(g, gsd, tmp_path):
    import instaorder_amd as ia
    path = os.path.join(str(tmp_path), "ckpt_iter_7.pth.tar")
    torch.save({"step": 7, "state_dict": {"module." + k: v for k, v in gsd.items()}, "optimizer": {}}, path)
    m = ia.PartialCompletionMask(dict(CFG))
    m.load_state(str(tmp_path), Iter=7)
    got = m.model.state_dict()
    for k, v in gsd.items():
        assert torch.equal(got["module." + k].cpu(), v), k
    assert ia.backbone.unet2 is unet.unet2 and callable(ia.backbone.unet025)


# ---- fold and layout -------------------------------------------------------------------------------------------------
def test_fold_equals_fp64_eval_batchnorm():
    torch.manual_seed(2)
    conv, bn = torch.nn.Conv2d(5, 7, 3, padding=1), torch.nn.BatchNorm2d(7)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5), bn.bias.normal_(0, 0.3), bn.running_mean.normal_(0, 0.3), bn.running_var.uniform_(0.5, 2.0)
    bn.eval()
    x = torch.randn(2, 5, 6, 9, dtype=torch.float64)
    w, b = unet.fold_conv_bn(conv, bn)
    ref = F.batch_norm(F.conv2d(x, conv.weight.double(), conv.bias.double(), padding=1), bn.running_mean.double(),
                       bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)
    assert rel_err(F.conv2d(x, w, b, padding=1).detach().numpy(), ref.detach().numpy()) < 1e-13


def emulate(net, co32, x):
    """the plan of unet.UNet.features on the CPU in fp64: the PACKED operands applied by F.conv2d to tensors in their
    stored layouts, plain pooling / interpolation / concatenation of the stored tensors, the packed head"""
    layers, (wo, bo, cs) = net.operands(co32)

    def conv(t, layer):
        wop, bias, ci_st, co_st, narrow = layer
        assert t.shape[1] == ci_st
        w = wop.double().permute(2, 0, 1) if narrow else wop.double()          # -> [Co][9][Ci]
        w = w.reshape(co_st, 3, 3, ci_st).permute(0, 3, 1, 2)
        return F.relu(F.conv2d(t, w, bias.double(), padding=1))

    t = torch.zeros(x.shape[0], net.input_stored(co32), *x.shape[2:], dtype=torch.float64)
    t[:, :2] = x
    t = conv(conv(t, layers[0]), layers[1])
    skips = [t]
    for b in range(1, 5):
        t = conv(conv(F.max_pool2d(t, 2), layers[2 * b]), layers[2 * b + 1])
        skips.append(t)
    t = skips.pop()
    for b in range(5, 9):
        x2 = skips.pop()
        t = torch.cat([x2, F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)], 1)
        t = conv(conv(t, layers[2 * b]), layers[2 * b + 1])
    return F.conv2d(t, wo.double().view(2, cs, 1, 1), bo.double()), t


@pytest.mark.parametrize("co32", [True, False])
@pytest.mark.parametrize("arch", ["unet025", "unet1", "unet2"])
def test_padded_concatenated_layout_maps_every_channel(arch, co32):
    """unet1's 16-channel tensors are stored as 32, so its concatenations carry a gap the filters must mirror"""
    sd = pr.seeded_state(arch, 5)
    net = getattr(unet, arch)(2)
    net.load_state_dict(sd, strict=True)
    net.eval()
    x = torch.from_numpy(np.random.RandomState(1).rand(2, 2, 16, 16) > 0.5).double()
    with torch.no_grad():
        got, last = emulate(net, co32, x)
        ref = pr.unet_forward(sd, x)
    # the operands are fp32 roundings of the fp64 fold: 19 layers of 6e-8 relative
    assert rel_err(got.numpy(), ref.numpy()) < 5e-6
    real = net.width[0]
    assert not last[:, real:].any(), "padding channels must stay exactly zero"
    if arch == "unet1" and co32:
        segs = [s[2] for s in net.plan(True)[0]]
        assert [(16, 32), (16, 32)] in segs, "the gap case is not exercised"


# ---- the order rule --------------------------------------------------------------------------------------------------
def test_order_rule_on_hand_made_matrices():
    occ = np.array([[0, 3, 0, 2],
                    [5, 0, 0, 2],
                    [0, 0, 0, 0],
                    [1, 2, 4, 0]], np.float32)
    want = np.array([[0, 1, 0, 0],       # [0,1]: 3 < 5 -> 1; [0,2]: both 0 -> 0; [0,3]: 2 > 1 -> 0
                     [0, 0, 0, 0],       # [1,0]: 5 > 3 -> 0; [1,3]: a tie -> untouched 0
                     [0, 0, 0, 1],       # [2,3]: 0 < 4 -> 1
                     [1, 0, 0, 0]])      # [3,0]: 1 < 2 -> 1; [3,2]: 4 > 0 -> 0
    got = inference.order_from_occ_values(occ)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(pr.order_rule(occ), want)
    assert not inference.order_from_occ_values(np.zeros((3, 3), np.float32)).any()


# ---- what is refused -------------------------------------------------------------------------------------------------
def test_refused_arguments():
    import instaorder_amd as ia
    m1 = np.zeros((2, 8, 8), np.uint8)
    args = (None, None, m1, np.ones(2), np.array([[0, 0, 8, 8]] * 2), "all")
    with pytest.raises(NotImplementedError, match="input_size"):
        inference.infer_order(*args, input_size=None)
    with pytest.raises(NotImplementedError, match="interp"):
        inference.infer_order(*args, input_size=32, interp="linear")
    with pytest.raises(NotImplementedError, match="dilate_kernel"):
        inference.infer_order(*args, input_size=32, dilate_kernel=3)
    with pytest.raises(NotImplementedError, match="use_rgb"):
        inference.infer_order(*args, input_size=32, use_rgb=True)
    with pytest.raises(ValueError, match="multiple of 16"):
        inference.infer_order(*args, input_size=40)
    net = unet.unet025(2)
    with pytest.raises(NotImplementedError, match="training mode"):
        net.train()(torch.zeros(1, 2, 16, 16))
    with pytest.raises(NotImplementedError, match="bf16"):
        unet.unet025(2, dtype="bf16").eval()(torch.zeros(1, 2, 16, 16))
    with pytest.raises(NotImplementedError, match="use_rgb"):
        ia.PartialCompletionMask(dict(CFG, use_rgb=True))
    m = ia.PartialCompletionMask(dict(CFG))
    with pytest.raises(NotImplementedError, match="training PCNet-M is not in the package yet"):
        m.step()
    z = torch.zeros(1, 1, 16, 16)
    with pytest.raises(ValueError, match="outside"):
        m.set_input(rgb=None, mask=z, eraser=z, target=torch.full((1, 16, 16), 255))
    with pytest.raises(KeyError):
        ia.SingleStageModel(dict(CFG, backbone_arch="unet3"))
