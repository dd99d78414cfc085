#!/usr/bin/env python3
"""Generate tests/golden/pcnet_train.npz by running the REAL reference's PCNet-M training step: ``PartialCompletionMask``
with ``unet025`` and the SGD of the ``pcnet_m`` config, two consecutive ``step()`` calls (the second one uses the
momentum buffer), once in the reference's fp32 and once with its modules cast to fp64.

Runs only where the reference is checked out (never on the GPU box).  The reference is imported unmodified, with the
shims of make_golden.py; its ``average_gradients`` wants a process group, so a one-rank gloo group is opened.

The weights are ``pcnet_ref.seeded_state("unet025", SEED)``; the input is N = 2 patches of 32 x 32 cut from a
``pcnet_ref.scene`` (``pcnet_train_ref.inputs``) with a seeded target.

Stored, in three files (pcnet_train.npz: inputs, settings and the fp32 records; pcnet_train_f64_1.npz / _2.npz: the fp64
records of step 1 / 2 -- one file would pass the 1 MiB cap of a committed file): the seed of the start state, the
inputs, and per precision P in (32, 64) and step s in (1, 2): the loss
("P/s/loss"), every parameter's gradient ("P/s/grad/<key>") and every parameter and buffer afterwards ("P/s/sd/<key>").

Two conditions are enforced, their figures printed:
  gradient condition  per tensor, rel_err(fp32 gradient, fp64 gradient) <= 1e-3 in both steps (the deepest BatchNorm sees
                      8 rows per channel; a seed on which it is ill-conditioned would let the GPU test pass anything);
  bias condition      max |conv bias.grad| <= 1e-5 max |that convolution's weight.grad|: the reference's gradient of a
                      bias in front of a batch-statistics BatchNorm is rounding noise, for which exact zeros stand in.

usage:  python tests/golden/make_golden_pcnet_train.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402
import pcnet_ref  # noqa: E402
import pcnet_train_ref as ptr  # noqa: E402
from helpers import rel_err  # noqa: E402

SEED = 11
INPUT_SEED = 21
INMASK_WEIGHT = 5.0


def run(models, cfg, sd, mask, eraser, target, double):
    torch.manual_seed(0)
    m = models.PartialCompletionMask(cfg, dist_model=False)
    m.model.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)
    if double:
        m.model.double()
    m.switch_to("train")
    dt = torch.float64 if double else torch.float32
    m.set_input(rgb=torch.zeros(mask.shape[0], 3, 32, 32), mask=mask.to(dt), eraser=eraser.to(dt), target=target)
    out = {}
    for s in (1, 2):
        loss = m.step()["loss"]
        tag = "%d/%d/" % (64 if double else 32, s)
        out[tag + "loss"] = np.asarray(loss.item(), np.float64)
        for k, p in m.model.named_parameters():
            out[tag + "grad/" + k[len("module."):]] = p.grad.detach().numpy().copy()
        for k, v in m.model.state_dict().items():
            out[tag + "sd/" + k[len("module."):]] = v.detach().numpy().copy()
    return out


def main():
    mg.install_shims()
    mg.init_dist(0, 1, 29731)
    import models
    cfg = dict(mg.load_cfg("pcnet_m")["model"])
    cfg["backbone_arch"] = "unet025"
    cfg["inmask_weight"] = INMASK_WEIGHT
    sd = pcnet_ref.seeded_state("unet025", SEED)
    mask, eraser, target = ptr.inputs(INPUT_SEED)
    out = {}           # (the start state is pcnet_ref.seeded_state("unet025", seed): the tests rebuild it from the seed)
    out.update(seed=np.int64(SEED), key_order=np.array(list(sd)), mask=mask.numpy(), eraser=eraser.numpy(), target=target.numpy(),
               inmask_weight=np.float64(INMASK_WEIGHT), lr=np.float64(cfg["lr"]), weight_decay=np.float64(cfg["weight_decay"]))
    out.update(run(models, cfg, sd, mask, eraser, target, False))
    out.update(run(models, cfg, sd, mask, eraser, target, True))

    params = [k for k in sd if ptr.is_param(k)]
    for s in (1, 2):
        worst = (0.0, "")
        for k in params:
            if ptr.is_conv_bias(k):
                continue
            e = rel_err(out["32/%d/grad/%s" % (s, k)], out["64/%d/grad/%s" % (s, k)])
            worst = max(worst, (e, k))
        print("step %d: gradient condition: worst e32 %.3e (%s), cap %.0e" % (s, worst[0], worst[1], ptr.GRAD_CAP))
        assert worst[0] <= ptr.GRAD_CAP, worst
        ratio = (0.0, "")
        for k in params:
            if ptr.is_conv_bias(k):
                for p in ("32", "64"):
                    b = np.abs(out["%s/%d/grad/%s" % (p, s, k)]).max()
                    w = np.abs(out["%s/%d/grad/%s" % (p, s, k[:-len("bias")] + "weight")]).max()
                    ratio = max(ratio, (float(b / w), p + ":" + k))
        print("step %d: bias condition: worst max|bias.grad| / max|weight.grad| %.3e (%s), cap 1e-5" % ((s,) + ratio))
        assert ratio[0] <= 1e-5, ratio
        print("step %d: loss fp32 %.9f fp64 %.12f" % (s, out["32/%d/loss" % s], out["64/%d/loss" % s]))
    share = float(eraser.mean())
    print("inputs: eraser share %.3f, mask share %.3f, target share %.3f" % (share, float(mask.mean()), float(target.float().mean())))
    # three files, each under the repository's 1 MiB cap for a committed file: the fp64 records are 8 bytes an element
    parts = {"pcnet_train": {k: v for k, v in out.items() if not k.startswith("64/")},
             "pcnet_train_f64_1": {k: v for k, v in out.items() if k.startswith("64/1/")},
             "pcnet_train_f64_2": {k: v for k, v in out.items() if k.startswith("64/2/")}}
    for name, part in parts.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20), path


if __name__ == "__main__":
    main()
