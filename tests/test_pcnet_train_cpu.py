"""PCNet-M training, the parts that need no GPU: the restatement of the training step (tests/pcnet_train_ref.py) against
two recorded steps of the real reference (tests/golden/pcnet_train*.npz), the conditions that golden must keep meeting,
and the stored-layout algebra of instaorder_amd.unet's training plan (filters, gamma and beta scattered to the
64-multiple layout by the package's own code, run through torch ops, gradients sliced back) against the real-shape step.

What is pinned to what: the restatement in fp64 is held to the reference's modules run in fp64 at 1e-9 per tensor (fp64
rounding through ~40 layers sits many orders below that; a wrong divisor, weight or statistic shows at 1e-3 or more); the
GPU tests then hold the package to the golden and to the restatement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcnet_ref as pr
import pcnet_train_ref as ptr
from helpers import load_golden, rel_err
from instaorder_amd import unet


@pytest.fixture(scope="module")
def g():
    out = {}
    for tag in ("pcnet_train", "pcnet_train_f64_1", "pcnet_train_f64_2"):
        z = load_golden(tag)
        out.update({k: z[k] for k in z.files})
    return out


def golden_inputs(g):
    return torch.from_numpy(g["mask"]), torch.from_numpy(g["eraser"]), torch.from_numpy(g["target"])


def test_golden_inputs_are_the_seeded_ones(g):
    sd = pr.seeded_state("unet025", int(g["seed"]))
    assert [str(k) for k in g["key_order"]] == list(sd)
    mask, eraser, target = ptr.inputs(21)
    assert np.array_equal(mask.numpy(), g["mask"]) and np.array_equal(eraser.numpy(), g["eraser"])
    assert np.array_equal(target.numpy(), g["target"])
    # both planes and both classes are present inside and outside the eraser
    er = g["eraser"][:, 0] == 1
    assert 0.05 < er.mean() < 0.5 and g["target"][er].min() == 0 and g["target"][er].max() == 1
    assert g["target"][~er].min() == 0 and g["target"][~er].max() == 1


def test_golden_conditions(g):
    """the gradient condition and the bias condition of make_golden_pcnet_train.py, on the stored records"""
    keys = [str(k) for k in g["key_order"] if ptr.is_param(str(k))]
    for s in (1, 2):
        worst = max(rel_err(g["32/%d/grad/%s" % (s, k)], g["64/%d/grad/%s" % (s, k)]) for k in keys if not ptr.is_conv_bias(k))
        ratio = 0.0
        for k in keys:
            if ptr.is_conv_bias(k):
                for p in ("32", "64"):
                    ratio = max(ratio, float(np.abs(g["%s/%d/grad/%s" % (p, s, k)]).max()
                                             / np.abs(g["%s/%d/grad/%s" % (p, s, k[:-4] + "weight")]).max()))
        print("step %d: worst e32 %.3e (cap %.0e), worst bias ratio %.3e (cap 1e-5)" % (s, worst, ptr.GRAD_CAP, ratio))
        assert worst <= ptr.GRAD_CAP and ratio <= 1e-5


def test_restatement_matches_the_reference_fp64(g):
    sd = ptr.cast_state(pr.seeded_state("unet025", int(g["seed"])), torch.float64)
    mask, eraser, target = golden_inputs(g)
    mom = {}
    for s in (1, 2):
        loss, grads = ptr.train_step(sd, mom, mask.double(), eraser.double(), target, float(g["inmask_weight"]), float(g["lr"]),
                                     float(g["weight_decay"]))
        ref = float(g["64/%d/loss" % s])
        assert abs(float(loss) - ref) <= 1e-9 * abs(ref), (s, float(loss), ref)
        for k, v in grads.items():
            r = g["64/%d/grad/%s" % (s, k)]
            if ptr.is_conv_bias(k):
                # the true gradient is 0; both sides hold fp64 rounding noise
                cap = 1e-9 * np.abs(g["64/%d/grad/%s" % (s, k[:-4] + "weight")]).max()
                assert np.abs(v.numpy()).max() <= cap and np.abs(r).max() <= cap, (s, k)
            else:
                assert rel_err(v.numpy(), r) <= 1e-9, (s, k, rel_err(v.numpy(), r))
        for k, v in sd.items():
            r = g["64/%d/sd/%s" % (s, k)]
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(r) == 100 + s, (s, k)
            else:
                assert rel_err(v.numpy(), r) <= 1e-9, (s, k, rel_err(v.numpy(), r))


# ---- the stored layout of the training plan ---------------------------------------------------------------------------
class TorchTrainOps(object):
    """the operator set of unet.UNet.features_train as torch functions on NHWC tensors of any float dtype"""

    @staticmethod
    def pack_input(m1, m2, cs):
        x = m1.new_zeros(m1.shape + (cs,))
        x[..., 0], x[..., 1] = m1, m2
        return x

    @staticmethod
    def conv_bn_relu(x, w, gamma, beta, rm, rv, route):
        y = F.conv2d(x.permute(0, 3, 1, 2), w, None, padding=1)
        y = F.relu(F.batch_norm(y, rm, rv, gamma, beta, True, 0.1, 1e-5))
        return y.permute(0, 2, 3, 1).contiguous()

    @staticmethod
    def max_pool_2x2(x):
        return F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous(), x

    @staticmethod
    def up2x_concat(x2, x1):
        up = F.interpolate(x1.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
        return torch.cat([x2, up.permute(0, 2, 3, 1)], 3).contiguous()


@pytest.mark.parametrize("arch", ["unet025", "unet1", "unet2"])
def test_stored_layout_step_equals_the_real_shape_step(arch):
    """Padding filters, gamma and beta are zero, so the padding channels hold exactly 0 forward and backward and every real
    channel computes what the real-shape network computes: gradients (sliced back to the parameters' shapes), the conv
    biases' exact zeros, the running estimates with the bias folded into the mean, the counters.  unet1 has the gap in the
    middle of the concatenation; unet2 has it in up4 only."""
    sd = pr.seeded_state(arch, 5)
    mask, eraser, target = ptr.inputs(23, n=2, size=16)
    net = getattr(unet, arch)(2)
    net.load_state_dict(sd, strict=True)
    net.double().train()
    segs = [s[2] for s in net.plan(False, cin=unet.TRAIN_INPUT)[0]]
    if arch != "unet025":
        c0 = net.width[0]
        assert [(c0, 64), (c0, 64)] in segs, "the gap case is not exercised"
    seen = []
    feat = net.features_train(mask[:, 0].double(), eraser[:, 0].double(), impl=TorchTrainOps)
    seen.append(feat)
    real = net.width[0]
    assert feat.shape[3] == 64 and not feat[..., real:].any(), "padding channels must stay exactly zero"
    logits = F.conv2d(feat[..., :real].permute(0, 3, 1, 2), net.outc.conv.weight, net.outc.conv.bias)
    loss = pr.masked_loss(logits, target, eraser[:, 0].double(), 5.0)
    feat.retain_grad()
    loss.backward()
    assert not feat.grad[..., real:].any(), "padding channels must receive exactly zero gradient"
    ref = ptr.cast_state(sd, torch.float64)
    rloss, rgrads = ptr.loss_and_grads(ref, mask.double(), eraser.double(), target, 5.0)
    assert abs(float(loss.detach()) - float(rloss)) <= 1e-9 * abs(float(rloss))
    got = dict(net.named_parameters())
    worst = 0.0
    for k, r in rgrads.items():
        gk = got[k].grad
        assert gk is not None and gk.shape == r.shape, (k, None if gk is None else tuple(gk.shape))
        if ptr.is_conv_bias(k):
            assert not gk.any(), k
        else:
            # equal as algebra; the CPU convolution adds a different number of (zero) terms in a different order, so the
            # fp64 roundings differ: held to the file's fp64 bar of 1e-9, where a misplaced channel shows at order 1
            e = rel_err(gk.numpy(), r.numpy())
            worst = max(worst, e)
            assert e <= 1e-9, (k, e)
    for k, v in net.state_dict().items():
        if not ptr.is_param(k):
            assert rel_err(v.numpy(), ref[k].numpy()) <= 1e-9, k
    print("%s: worst gradient distance of the stored-layout step from the real-shape step %.2e" % (arch, worst))


def test_bn_route_is_decided_by_rows():
    assert unet.UNet.bn_route(2048) == "fused" and unet.UNet.bn_route(128) == "fused"
    assert unet.UNet.bn_route(32) == "split" and unet.UNet.bn_route(8) == "split" and unet.UNet.bn_route(192) == "split"


def test_what_training_still_refuses():
    import instaorder_amd as ia
    cfg = dict(algo="PartialCompletionMask", backbone_arch="unet025", backbone_param=dict(in_channels=2, n_classes=2),
               use_rgb=False, inmask_weight=5.0, optim="SGD", lr=1e-3, weight_decay=1e-4)
    with pytest.raises(NotImplementedError, match="cuda tensor"):
        unet.unet025(2).train()(torch.zeros(1, 2, 16, 16))
    with pytest.raises(NotImplementedError, match="bf16"):
        unet.unet025(2, dtype="bf16").train()(torch.zeros(1, 2, 16, 16))
    with pytest.raises(NotImplementedError, match="bf16"):
        ia.PartialCompletionMask(dict(cfg, dtype="bf16")).step()
    with pytest.raises(NotImplementedError, match="set_input"):
        ia.PartialCompletionMask(dict(cfg)).step()
    net = unet.unet025(2).train()
    with pytest.raises(RuntimeError, match="eval mode"):
        net.features(torch.zeros(1, 16, 16), torch.zeros(1, 16, 16))


def test_restatement_at_given_decisions():
    """fed its own decisions the restatement computes what it computes without; a decision flipped far from the knife edge
    is counted as a violation, so a wrong mask cannot hide behind the rule"""
    sd = pr.seeded_state("unet025", 5)
    mask, eraser, target = ptr.inputs(23, n=2, size=16)
    rec = {"relu": [], "pool": []}
    relu, pool = F.relu, F.max_pool2d
    try:
        F.relu = lambda x, *a, **k: (rec["relu"].append(x.detach() > 0), relu(x))[1]
        F.max_pool2d = lambda x, *a, **k: (rec["pool"].append(ptr._first_max(ptr.windows(x.detach()))), pool(x, 2))[1]
        l0, g0 = ptr.loss_and_grads(ptr.cast_state(sd, torch.float64), mask.double(), eraser.double(), target, 5.0)
    finally:
        F.relu, F.max_pool2d = relu, pool
    assert len(rec["relu"]) == 18 and len(rec["pool"]) == 4
    own = dict(rec)
    l1, g1 = ptr.loss_and_grads(ptr.cast_state(sd, torch.float64), mask.double(), eraser.double(), target, 5.0, decisions=own)
    assert float(l1) == float(l0) and own["differing"] == 0 and own["violations"] == 0
    assert all(torch.equal(g1[k], g0[k]) for k in g0)
    bad = dict(rec, relu=[~m if i == 16 else m for i, m in enumerate(rec["relu"])],
               pool=[(p + 1) % 4 if i == 0 else p for i, p in enumerate(rec["pool"])])
    ptr.loss_and_grads(ptr.cast_state(sd, torch.float64), mask.double(), eraser.double(), target, 5.0, decisions=bad)
    assert bad["differing"] > 1000 and bad["violations"] > 0.5 * bad["differing"]
