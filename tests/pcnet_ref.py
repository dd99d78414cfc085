"""Restatement of PCNet-M evaluation for the tests: the UNet of models/backbone/unet in eval mode as plain torch-CPU
functions on a state dict (any float dtype; the tests use fp64), MaskWeightedCrossEntropyLoss, and the dual-completion
``infer_order`` with numpy crops and the nearest-neighbour rule of oracle/preprocess_oracle.py.  Written from the
behaviour of the reference, held to a run of the real reference by tests/golden/pcnet.npz (tests/test_pcnet_cpu.py).
Also: the seeded weights every PCNet-M test uses, the synthetic scenes, and the "undecided pixel" rule.

Undecided pixels.  The completion is softmax(l)[1] > th, i.e. d = l1 - l0 > ln(th / (1 - th)).  An fp32 evaluation whose
logits are within ``bar * max|logits|`` of the fp64 ones moves d by at most twice that, so a pixel with
|d - ln(th / (1 - th))| <= 2 * bar * max|logits| may legitimately fall on either side: it is *undecided*.  Every other
pixel must match, and a patch's count may differ by at most its number of undecided pixels under the eraser.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import preprocess_oracle as pre  # noqa: E402

BAR = 2e-5                     # the project's single-launch bar: max|got - ref| / max|ref|
WIDTHS = {"unet025": 0.25, "unet05": 0.5, "unet1": 1, "unet2": 2, "unet4": 4}
BLOCKS = ["inc.conv"] + ["down%d.mpconv.1" % i for i in range(1, 5)] + ["up%d.conv" % i for i in range(1, 5)]


def state_shapes(arch, in_channels=2, n_classes=2):
    """key -> shape of the reference's UNet state dict, in its order"""
    w = WIDTHS[arch]
    c = [int(16 * w), int(32 * w), int(64 * w), int(128 * w)]
    io = [(in_channels, c[0]), (c[0], c[1]), (c[1], c[2]), (c[2], c[3]), (c[3], c[3]), (2 * c[3], c[2]), (2 * c[2], c[1]),
          (2 * c[1], c[0]), (2 * c[0], c[0])]
    shapes = {}
    for name, (ci, co) in zip(BLOCKS, io):
        for k, cin in ((0, ci), (3, co)):
            p = "%s.conv.%d." % (name, k)
            q = "%s.conv.%d." % (name, k + 1)
            shapes[p + "weight"], shapes[p + "bias"] = (co, cin, 3, 3), (co,)
            shapes[q + "weight"], shapes[q + "bias"] = (co,), (co,)
            shapes[q + "running_mean"], shapes[q + "running_var"], shapes[q + "num_batches_tracked"] = (co,), (co,), ()
    shapes["outc.conv.weight"], shapes["outc.conv.bias"] = (n_classes, c[0], 1, 1), (n_classes,)
    return shapes


def seeded_state(arch, seed):
    """He-normal filters, biases ~ N(0, 0.1), BatchNorm gamma in [0.5, 1.5], beta and running mean ~ N(0, 0.1), running
    variance in [0.5, 1.5]: activations of order 1 at every depth (the reference's xavier(0.02) start gives logits of
    1e-12, on which no test could see anything)."""
    rng = np.random.RandomState(seed)
    sd = {}
    for k, shp in state_shapes(arch).items():
        if k.endswith("num_batches_tracked"):
            v = np.array(100, np.int64)
        elif len(shp) == 4:
            v = rng.randn(*shp) * math.sqrt(2.0 / (shp[1] * shp[2] * shp[3]))
        elif k.endswith("running_var") or (k.endswith("weight") and len(shp) == 1):
            v = rng.uniform(0.5, 1.5, shp)
        else:
            v = rng.randn(*shp) * 0.1
        sd[k] = torch.from_numpy(np.asarray(v, np.int64 if k.endswith("tracked") else np.float32))
    return sd


def unet_forward(sd, x):
    """x [N,2,S,S] -> logits [N,2,S,S] in x's dtype; eval-mode BatchNorm"""
    dt = x.dtype
    g = lambda k: sd[k].to(dt)          # noqa: E731

    def double_conv(x, name):
        for k in (0, 3):
            p, q = "%s.conv.%d." % (name, k), "%s.conv.%d." % (name, k + 1)
            x = F.conv2d(x, g(p + "weight"), g(p + "bias"), padding=1)
            x = F.batch_norm(x, g(q + "running_mean"), g(q + "running_var"), g(q + "weight"), g(q + "bias"), False, 0.1, 1e-5)
            x = F.relu(x)
        return x

    xs = [double_conv(x, BLOCKS[0])]
    for name in BLOCKS[1:5]:
        xs.append(double_conv(F.max_pool2d(xs[-1], 2), name))
    y = xs.pop()
    for name in BLOCKS[5:]:
        x2 = xs.pop()
        y = F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=True)
        assert y.shape[2:] == x2.shape[2:], "the patch side is no multiple of 16"
        y = double_conv(torch.cat([x2, y], 1), name)
    return F.conv2d(y, g("outc.conv.weight"), g("outc.conv.bias"))


def masked_loss(logits, target, eraser, inmask_weight):
    """MaskWeightedCrossEntropyLoss: logits [N,2,H,W], target [N,H,W] in {0, 1}, eraser [N,H,W]"""
    n, _, h, w = logits.shape
    ce = F.cross_entropy(logits, target.long(), reduction="none")
    inside = eraser != 0
    return (inmask_weight * ce[inside].sum() + ce[~inside].sum()) / (n * h * w)


def masked_loss_as_reference(logits, target, eraser, inmask_weight):
    """the same loss in the reference's order of operations (rows gathered inside / outside the eraser, one summed
    cross-entropy each), so that an fp32 evaluation rounds as the reference's does"""
    n, c, h, w = logits.shape
    inside = eraser != 0
    rows = logits.permute(0, 2, 3, 1).contiguous()
    loss_in = F.cross_entropy(rows[inside].view(-1, c), target[inside].long(), reduction="sum")
    loss_out = F.cross_entropy(rows[~inside].view(-1, c), target[~inside].long(), reduction="sum")
    return (inmask_weight * loss_in + 1.0 * loss_out) / (n * h * w)


def logit_threshold(th):
    return math.log(th / (1.0 - th))


def order_rule(occ_value):
    order = np.zeros(occ_value.shape, dtype=np.int64)
    order[occ_value > occ_value.T] = 0
    order[occ_value < occ_value.T] = 1
    order[(occ_value == 0) & (occ_value == 0).T] = 0
    return order


def bordering(a, b):
    a = np.asarray(a) == 1
    d = a.copy()
    d[1:] |= a[:-1]
    d[:-1] |= a[1:]
    d[:, 1:] |= a[:, :-1]
    d[:, :-1] |= a[:, 1:]
    return bool(np.any(d & (np.asarray(b) != 0)))


def pair_index(inmodal, pairs):
    n = inmodal.shape[0]
    ind = []
    for i in range(n):
        for j in range(i + 1, n):
            if pairs == "nbor" and not bordering(inmodal[i], inmodal[j]):
                continue
            ind += [[i, j], [j, i]]
    return np.array(ind, np.int64).reshape(-1, 2)


def patches(inmodal, bboxes, ind, input_size):
    """(erased target patches, eraser patches) uint8 [P,S,S]: both cropped by the target's box, nearest-resized"""
    tp, ep = [], []
    for t, e in ind:
        a = pre.resize(pre.crop_padding(inmodal[t], bboxes[t]), (input_size, input_size), pre.INTER_NEAREST).copy()
        b = pre.resize(pre.crop_padding(inmodal[e], bboxes[t]), (input_size, input_size), pre.INTER_NEAREST)
        a[b == 1] = 0
        tp.append(a)
        ep.append(b)
    return np.stack(tp), np.stack(ep)


def infer_order(sd, inmodal, category, bboxes, pairs="all", th=0.5, input_size=32, bar=BAR, as_reference=False):
    """-> dict(order, occ_value, ind, target, eraser, comp, logits ([P,2,S,S]), counts, undecided (per patch, under
    the eraser), undecided_map).  Default: one fp64 forward over all patches, the threshold taken on the logit difference
    (the anchor of the GPU tests and of the undecided rule).  ``as_reference``: the reference's own arithmetic -- fp32, one
    patch per forward, softmax(l)[1] > th -- which reproduces its thresholded outputs bit for bit."""
    inmodal, bboxes = np.asarray(inmodal), np.asarray(bboxes)
    n = inmodal.shape[0]
    ind = pair_index(inmodal, pairs)
    occ = np.zeros((n, n), np.float32)
    if len(ind) == 0:
        return dict(order=order_rule(occ), occ_value=occ, ind=ind)
    tp, ep = patches(inmodal, bboxes, ind, input_size)
    cat = np.asarray(category, np.float64)[ind[:, 0]]
    x = torch.from_numpy(np.stack([tp.astype(np.float64) * cat[:, None, None], ep.astype(np.float64)], 1))
    with torch.no_grad():
        if as_reference:
            logits = torch.cat([unet_forward(sd, x[k:k + 1].float()) for k in range(len(x))])
            comp = (F.softmax(logits, dim=1)[:, 1] > th).numpy().astype(np.uint8)
        else:
            logits = unet_forward(sd, x)
    d = (logits[:, 1] - logits[:, 0]).double().numpy() - logit_threshold(th)
    if not as_reference:
        comp = (d > 0).astype(np.uint8)
    und = (np.abs(d) <= 2 * bar * float(logits.abs().max())) & (ep == 1)
    counts = ((comp > tp) & (ep == 1)).sum((1, 2))
    ratio2 = np.array([(bboxes[t, 2] / float(input_size)) ** 2 for t, _ in ind])
    for k, (t, e) in enumerate(ind):
        occ[t, e] = counts[k] * ratio2[k]
    return dict(order=order_rule(occ), occ_value=occ, ind=ind, ratio2=ratio2, target=tp, eraser=ep, comp=comp, logits=logits, counts=counts,
                undecided=und.sum((1, 2)), undecided_map=und)


def calibrate_outc_bias(sd, inmodal_scenes, th=0.5):
    """shift outc.bias so that the median of l1 - l0 - ln(th / (1 - th)) under the erasers of the given scenes
    [(inmodal, category, bboxes, input_size)] is 0: half of the eraser pixels complete.  Without it random weights complete
    almost all pixels or almost none and every order test is vacuous."""
    ds = []
    for inmodal, category, bboxes, size in inmodal_scenes:
        r = infer_order(sd, inmodal, category, bboxes, "all", th, size)
        d = (r["logits"][:, 1] - r["logits"][:, 0]).numpy() - logit_threshold(th)
        ds.append(d[r["eraser"] == 1])
    shift = float(np.median(np.concatenate(ds)))
    sd = dict(sd)
    b = sd["outc.conv.bias"].clone().double()
    b[1] -= shift
    sd["outc.conv.bias"] = b.float()
    return sd


def scene(seed, n, H, W, box_side, jitter=0):
    """n overlapping ellipses (instance i drawn over the earlier ones: visible masks, values 1), their categories, and
    square xywh boxes of side box_side (+- jitter) around them, some reaching outside the image."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    owner = np.full((H, W), -1)
    cen = []
    for i in range(n):
        cy, cx = rng.uniform(0.25 * H, 0.75 * H), rng.uniform(0.2 * W, 0.8 * W)
        ry, rx = rng.uniform(0.18, 0.32) * box_side, rng.uniform(0.18, 0.32) * box_side
        owner[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = i
        cen.append((cy, cx))
    inmodal = np.stack([(owner == i).astype(np.uint8) for i in range(n)])
    boxes = []
    for cy, cx in cen:
        s = box_side + (int(rng.randint(-jitter, jitter + 1)) if jitter else 0)
        boxes.append([int(cx - s / 2), int(cy - s / 2), s, s])
    return inmodal, np.ones(n, np.int64), np.array(boxes)


def fixture_conditions(r):
    """The figures of the three conditions every golden / restatement scene must meet -> (completed share under the
    erasers, undecided share of the eraser pixels, whether some pair's two occ values differ by more than what its
    undecided pixels could move them)"""
    er = r["eraser"] == 1
    share = float((r["comp"][er] == 1).mean())
    und = float(r["undecided"].sum()) / float(er.sum())
    occ = r["occ_value"]
    slack = np.zeros(occ.shape)
    for k, (t, e) in enumerate(r["ind"]):
        slack[t, e] = r["undecided"][k] * r["ratio2"][k]
    ok = bool((np.abs(occ.astype(np.float64) - occ.T) > slack + slack.T + 1e-6).any())
    return share, und, ok


# ---- the scenes of the restatement-only tests (non-identity resizes: held to this file, not to the reference) ---------
REST_SEED = 31               # seeded unet025 weights, calibrated on the scenes below that have pairs


def restatement_scenes():
    """tag -> (inmodal, category, bboxes, input_size, pairs)"""
    out = {}
    m, c, b = scene(41, 5, 96, 112, 48, jitter=6)             # boxes larger than the input size: the resize drops pixels
    out["larger"] = (m, c, b, 32, "all")
    m, c, b = scene(42, 5, 64, 64, 22, jitter=3)              # boxes smaller than the input size: pixels repeat
    out["smaller"] = (m, c + np.arange(5) % 2, b, 32, "all")  # (and categories 1 / 2: the input scale)
    m, c, b = scene(43, 5, 72, 88, 40, jitter=4)
    b = b.copy()
    b[0, 0], b[1, 1] = -25, 50                                # partly outside on the left / at the bottom
    b[4, :2] = (300, 300)                                     # wholly outside: empty patches, count 0
    out["outside"] = (m, c, b, 32, "all")
    m, c, b = scene(44, 4, 80, 160, 36, jitter=2)             # 'nbor' with an isolated instance in the right margin
    iso = np.zeros((1,) + m.shape[1:], np.uint8)
    iso[0, 10:22, 146:158] = 1
    m = np.concatenate([m * (1 - iso), iso])
    m[:, :, 130:146] = 0                                      # (a clear gap, so that nothing borders it)
    out["nbor"] = (m, np.ones(5, np.int64), np.concatenate([b, [[134, 0, 36, 36]]]), 32, "nbor")
    m, c, b = scene(45, 1, 48, 48, 32)
    out["single"] = (m, c, b, 32, "all")
    return out


def restatement_state():
    sc = restatement_scenes()
    cal = [(v[0], v[1], v[2], v[3]) for k, v in sc.items() if k in ("larger", "smaller", "outside")]
    return calibrate_outc_bias(seeded_state("unet025", REST_SEED), cal)
