#!/usr/bin/env python3
"""Generate tests/golden/pcnet.npz by running the REAL reference's PCNet-M: ``PartialCompletionMask`` with ``unet025``,
``forward_only`` and ``inference.infer_order(..., debug_info=True)``.

Runs only where the reference is checked out (never on the GPU box).  The reference is imported unmodified, with the
shims of make_golden.py (no GPU, no cv2 / torchvision here).  The shimmed ``cv2.resize`` is the identity and refuses
anything else, so the golden scenes use boxes of side exactly ``input_size`` (32 and 64): non-identity resizes are held to
the restatement (tests/pcnet_ref.py, the nearest rule of oracle/preprocess_oracle.py) only -- the standing caveat of
DESIGN "f3".

The reference's xavier(0.02) weights are overwritten with the seeded weights of ``pcnet_ref.seeded_state`` (He-normal
filters, order-1 BatchNorm terms), then ``outc.bias`` is shifted so that the median logit difference under the erasers
of the golden scenes is 0 (``pcnet_ref.calibrate_outc_bias``): half of the eraser pixels complete.  Without the shift
random weights complete almost all pixels or almost none and the order matrices say nothing.

Stored: the state dict ("sd/<key>"), the forward_only inputs and the reference's logits / loss / comp, per scene the
masks, categories, boxes and the reference's order matrix, pair index, three patch lists and the occ values formed from
them by the reference's expression, the forward_only logits and loss once more from the reference's modules cast to
fp64, and the sorted "key shape dtype" lists of the unet025 and unet2 state dicts.

usage:  python tests/golden/make_golden_pcnet.py
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

SEED = 11
SCENES = [("s32", 21, 6, 80, 96, 32), ("s64", 22, 6, 128, 160, 64)]      # tag, seed, instances, H, W, input_size
INMASK_WEIGHT = 5.0


def key_list(sd):
    return np.array(sorted("%s %s %s" % (k, ",".join(str(d) for d in v.shape), str(v.dtype).replace("torch.", ""))
                           for k, v in sd.items()))


def main():
    mg.install_shims()
    import inference as ref_infer
    import models
    cfg = dict(mg.load_cfg("pcnet_m")["model"])
    cfg["backbone_arch"] = "unet025"
    torch.manual_seed(0)
    m = models.PartialCompletionMask(cfg, dist_model=False)
    m.switch_to("eval")
    scenes = {tag: pcnet_ref.scene(seed, n, H, W, size) + (size,) for tag, seed, n, H, W, size in SCENES}
    sd = pcnet_ref.calibrate_outc_bias(pcnet_ref.seeded_state("unet025", SEED), list(scenes.values()))
    assert [k for k in m.model.state_dict()] == ["module." + k for k in sd], "key order differs from the reference's"
    m.model.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)
    out = {"sd/" + k: v.numpy() for k, v in sd.items()}
    out["keys_unet025"] = key_list(m.model.state_dict())
    out["keys_unet2"] = key_list(models.backbone.unet2(2, n_classes=2).state_dict())
    out["key_order"] = np.array(list(sd))
    out["inmask_weight"] = np.float64(INMASK_WEIGHT)

    # forward_only: three patches of the first scene (visible mask, eraser) with a seeded target
    r = pcnet_ref.infer_order(sd, *scenes["s32"][:3], "all", 0.5, 32)
    pick = [0, 7, 12]
    mask = r["target"][pick].astype(np.float32)[:, None]
    eraser = r["eraser"][pick].astype(np.float32)[:, None]
    target = ((mask[:, 0] > 0) | ((eraser[:, 0] == 1) & (np.random.RandomState(3).rand(3, 32, 32) < 0.5))).astype(np.int64)
    m.set_input(rgb=torch.zeros(3, 3, 32, 32), mask=torch.from_numpy(mask), eraser=torch.from_numpy(eraser),
                target=torch.from_numpy(target))
    ret, loss = m.forward_only(ret_loss=True)
    with torch.no_grad():
        logits = m.model(torch.cat([m.mask, m.eraser], dim=1))
    # the same two figures from the reference's modules run in fp64: what the fp64 restatement is held to at 1e-12
    m.model.double()
    with torch.no_grad():
        logits64 = m.model(torch.cat([m.mask, m.eraser], dim=1).double())
        loss64 = m.criterion(logits64, m.target, m.eraser.squeeze(1))
    m.model.float()
    out.update(fo_logits64=logits64.numpy(), fo_loss64=np.float64(loss64.item()))
    out.update(fo_mask=mask, fo_eraser=eraser, fo_target=target, fo_logits=logits.numpy(), fo_loss=np.float32(loss["loss"].item()),
               fo_comp=ret["mask_tensors"][2].numpy(), fo_vis_combo=ret["mask_tensors"][1].numpy(),
               fo_vis_target=ret["mask_tensors"][3].numpy())

    for tag, (inmodal, category, bboxes, size) in scenes.items():
        image = np.zeros(inmodal.shape[1:] + (3,), np.uint8)
        order, ind, tp, ep, ap = ref_infer.infer_order(m, image, inmodal, category, bboxes, pairs="all", use_rgb=False, th=0.5,
                                                       dilate_kernel=0, input_size=size, min_input_size=16, interp="nearest",
                                                       debug_info=True)
        occ = np.zeros(order.shape, dtype=np.float32)
        for i, idx in enumerate(ind):                     # the expression of inference.py:679-681 on the returned patches
            occ[idx[0], idx[1]] = ((ap[i] > tp[i]) & (ep[i] == 1)).sum() * ((bboxes[idx[0], 2] / float(size)) ** 2)
        out.update({tag + "/inmodal": inmodal, tag + "/category": category, tag + "/bboxes": bboxes,
                    tag + "/input_size": np.int64(size), tag + "/order": np.asarray(order, np.int64), tag + "/ind": ind,
                    tag + "/target": np.stack(tp).astype(np.uint8), tag + "/eraser": np.stack(ep).astype(np.uint8),
                    tag + "/comp": np.stack(ap).astype(np.uint8), tag + "/occ_value": occ})
        share, und, ok = pcnet_ref.fixture_conditions(pcnet_ref.infer_order(sd, inmodal, category, bboxes, "all", 0.5, size))
        print("%s: completed share %.3f, undecided share %.5f, decisive pair %s, order sum %d" % (tag, share, und, ok,
                                                                                                int(np.sum(order))))
    path = os.path.join(HERE, "pcnet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
