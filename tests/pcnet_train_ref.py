"""Restatement of the PCNet-M training step for the tests: the UNet of models/backbone/unet in TRAIN mode as plain torch-CPU
functions on a state dict (batch-statistics BatchNorm that advances the running estimates, biased convolutions),
MaskWeightedCrossEntropyLoss over world_size, and torch.optim.SGD's rule (momentum 0.9, coupled weight decay on every
parameter, momentum buffer = first decayed gradient).  Written from the behaviour of the reference
(models/partial_completion_mask.py:116-126), held to two recorded steps of the real reference by
tests/golden/pcnet_train.npz (tests/test_pcnet_train_cpu.py).  Also: the seeded inputs the training tests share.
"""
import numpy as np
import torch
import torch.nn.functional as F

import pcnet_ref as pr

MOMENTUM = 0.9
GRAD_CAP = 1e-3            # a fixture is usable only while the fp32 step's gradients stay this close to the fp64 step's


def is_param(k):
    return not k.endswith(("running_mean", "running_var", "num_batches_tracked"))


def is_conv_bias(k):
    """the bias of a 3x3 convolution in front of a BatchNorm: its true gradient is 0 (the batch mean removes it)"""
    return k.endswith((".conv.0.bias", ".conv.3.bias"))


def cast_state(sd, dt):
    """a private copy of the state: float tensors in ``dt``, the step counters as they are"""
    return {k: (v.clone() if k.endswith("num_batches_tracked") else v.detach().to(dt).clone()) for k, v in sd.items()}


def _first_max(win):
    """index (0..3, row-major) of the first maximum of each 2x2 window; win [...,4]"""
    eq = win == win.max(-1, keepdim=True).values
    three = torch.full(eq.shape[:-1], 3, dtype=torch.int64, device=win.device)
    return torch.where(eq[..., 0], 0 * three, torch.where(eq[..., 1], three - 2, torch.where(eq[..., 2], three - 1, three)))


def windows(a):
    """[N,C,H,W] -> the 2x2 windows [N,C,H/2,W/2,4], row-major inside a window"""
    n, c, h, w = a.shape
    return a.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)


def unet_train_forward(sd, x, decisions=None):
    """x [N,2,S,S] -> logits [N,2,S,S]; BatchNorm on batch statistics, sd's running estimates and counters advanced in
    place (momentum 0.1, unbiased variance).  Parameters of sd that require a gradient get one from the result.

    ``decisions`` = dict(relu=[bool [N,C,H,W] per unit], pool=[int64 [N,C,H/2,W/2] per pooling]): the network is evaluated
    with THESE ReLU masks and pool choices instead of its own (the gradient of a piecewise-linear network is defined per
    set of decisions; another fp32 arithmetic may take a knife-edge one the other way).  A decision may differ from the
    network's own only where it is undecided at the project's single-launch bar: |pre-activation| <= BAR max|layer|, or
    the chosen element within BAR max|layer| of the window's maximum.  decisions["differing"] gets the number of decisions
    that differ, decisions["violations"] the number of those that are not undecided (a test asserts it is 0)."""
    it = {"relu": 0, "pool": 0}
    if decisions is not None:
        decisions.setdefault("differing", 0)
        decisions.setdefault("violations", 0)

    def relu(z):
        if decisions is None:
            return F.relu(z)
        mask = decisions["relu"][it["relu"]]
        it["relu"] += 1
        diff = mask != (z.detach() > 0)
        decisions["differing"] += int(diff.sum())
        decisions["violations"] += int((diff & (z.detach().abs() > pr.BAR * z.detach().abs().max())).sum())
        return z * mask.to(z.dtype)

    def pool(a):
        if decisions is None:
            return F.max_pool2d(a, 2)
        idx = decisions["pool"][it["pool"]]
        it["pool"] += 1
        win = windows(a)
        out = win.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
        diff = idx != _first_max(win.detach())
        decisions["differing"] += int(diff.sum())
        short = win.detach().max(-1).values - out.detach()
        decisions["violations"] += int((diff & (short > pr.BAR * a.detach().abs().max())).sum())
        return out

    def double_conv(x, name):
        for k in (0, 3):
            p, q = "%s.conv.%d." % (name, k), "%s.conv.%d." % (name, k + 1)
            x = F.conv2d(x, sd[p + "weight"], sd[p + "bias"], padding=1)
            x = F.batch_norm(x, sd[q + "running_mean"], sd[q + "running_var"], sd[q + "weight"], sd[q + "bias"], True, 0.1, 1e-5)
            sd[q + "num_batches_tracked"] += 1
            x = relu(x)
        return x

    xs = [double_conv(x, pr.BLOCKS[0])]
    for name in pr.BLOCKS[1:5]:
        xs.append(double_conv(pool(xs[-1]), name))
    y = xs.pop()
    for name in pr.BLOCKS[5:]:
        x2 = xs.pop()
        y = F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=True)
        y = double_conv(torch.cat([x2, y], 1), name)
    return F.conv2d(y, sd["outc.conv.weight"], sd["outc.conv.bias"])


def loss_and_grads(sd, mask, eraser, target, inmask_weight, world_size=1, as_reference=False, decisions=None):
    """One forward + backward from ``sd`` (its BatchNorm buffers advance): -> (loss, {parameter key: gradient}).
    mask, eraser: [N,1,S,S] in sd's dtype; target [N,S,S] int64."""
    for k, v in sd.items():
        if is_param(k):
            v.requires_grad_(True)
            v.grad = None
    logits = unet_train_forward(sd, torch.cat([mask, eraser], 1), decisions)
    fn = pr.masked_loss_as_reference if as_reference else pr.masked_loss
    loss = fn(logits, target, eraser[:, 0], inmask_weight) / world_size
    loss.backward()
    grads = {}
    for k, v in sd.items():
        if is_param(k):
            grads[k] = v.grad.detach().clone()
            v.grad = None
            v.requires_grad_(False)
    return loss.detach(), grads


def sgd_update(sd, mom, grads, lr, weight_decay, momentum=MOMENTUM):
    """torch.optim.SGD on every parameter of sd, in place; ``mom``: key -> momentum buffer (empty before the first step)"""
    with torch.no_grad():
        for k, g in grads.items():
            d = g + weight_decay * sd[k]
            mom[k] = d.clone() if k not in mom else mom[k] * momentum + d
            sd[k] -= lr * mom[k]


def train_step(sd, mom, mask, eraser, target, inmask_weight, lr, weight_decay, world_size=1, as_reference=False, decisions=None):
    loss, grads = loss_and_grads(sd, mask, eraser, target, inmask_weight, world_size, as_reference, decisions)
    sgd_update(sd, mom, grads, lr, weight_decay)
    return loss, grads


def inputs(seed, n=2, size=32):
    """n (visible mask, eraser) patches of side ``size`` cut from a pcnet_ref.scene as make_golden_pcnet.py cuts them, and a
    seeded target: -> mask [n,1,S,S] fp32, eraser [n,1,S,S] fp32, target [n,S,S] int64"""
    inmodal, category, bboxes = pr.scene(seed, 6, 80, 96, size)
    ind = pr.pair_index(inmodal, "all")
    tp, ep = pr.patches(inmodal, bboxes, ind, size)
    area = (ep == 1).sum((1, 2)) * (tp == 1).sum((1, 2))
    pick = np.argsort(-area, kind="stable")[:n]                 # the patches with the most of both planes
    mask = tp[pick].astype(np.float32)[:, None]
    eraser = ep[pick].astype(np.float32)[:, None]
    rnd = np.random.RandomState(seed + 1).rand(n, size, size) < 0.5
    target = ((mask[:, 0] > 0) | ((eraser[:, 0] == 1) & rnd)).astype(np.int64)
    return torch.from_numpy(mask), torch.from_numpy(eraser), torch.from_numpy(target)


def gap32(sd, mask, eraser, target, inmask_weight):
    """per-parameter max-norm distance of the fp32 step's gradients from the fp64 step's (pcnet_ref's measure), the fp64
    loss and gradients: what the GPU bound max(3 e32, BAR) is made of"""
    from helpers import rel_err
    l64, g64 = loss_and_grads(cast_state(sd, torch.float64), mask.double(), eraser.double(), target, inmask_weight)
    l32, g32 = loss_and_grads(cast_state(sd, torch.float32), mask, eraser, target, inmask_weight, as_reference=True)
    e32 = {k: rel_err(g32[k].numpy(), g64[k].numpy()) for k in g64 if not is_conv_bias(k)}
    return e32, abs(float(l32) - float(l64)) / abs(float(l64)), l64, g64
