"""PartialCompletionMask (PCNet-M): evaluation of a checkpoint and the training step (models/partial_completion_mask.py:12-126).

``set_input(rgb, mask, eraser, target)`` + ``forward_only(ret_loss=True)`` reproduce the reference's validation pass: the
UNet on cat([mask, eraser]), ``comp`` = argmax with the visible mask pasted outside the eraser, and
MaskWeightedCrossEntropyLoss (models/losses.py:60-88)

    loss = (inmask_weight * CE_in + CE_out) / (n * h * w) / world_size

with CE_in / CE_out the cross-entropy SUMS over the pixels inside / outside the eraser -- two numbers the head kernel
returns (io_unet_head, loss mode; per-block partials added in a fixed order).  The order-recovery rule on top of the same
network is ``inference.infer_order``.  ``step()`` is the reference's training step, eager and fp32: the train-mode UNet of
unet.py (autograd nodes of ops.py), the same loss through the fused head node (io_unet_head forward, io_unet_head_bwd
backward), then the optimiser of SingleStageModel (FlatSGD / FlatAdam, ``clip_grad_norm``).  ``forward_only`` wants eval
mode (the reference's trainer switches before it validates).  The eraser-synthesising dataset and amodal completion are
not in the package.  The optimiser and the checkpoint I/O come from SingleStageModel unchanged.
"""
import torch

from . import distributed_utils
from .single_stage_model import SingleStageModel


class PartialCompletionMask(SingleStageModel):
    def __init__(self, params, load_pretrain=None, dist_model=False):
        if params.get("use_rgb", False):
            raise NotImplementedError("PartialCompletionMask: use_rgb=True is not in the package (the reference's "
                                      "UNet.forward(x) takes no image either).")
        super(PartialCompletionMask, self).__init__(params, dist_model)
        self.inmask_weight = float(params["inmask_weight"])
        if load_pretrain is not None:
            self.load_pretrain(load_pretrain)

    def set_input(self, rgb=None, mask=None, eraser=None, target=None):
        t = torch.as_tensor(target)
        lo, hi = (int(v) for v in torch.aminmax(t)) if t.numel() else (0, 0)
        if lo < 0 or hi > 1:
            raise ValueError("PartialCompletionMask.set_input: target holds values outside {0, 1} (min %d, max %d); "
                             "cross_entropy over 2 classes has no such class" % (lo, hi))
        dev = next(self.model.parameters()).device
        self.rgb = None if rgb is None else torch.as_tensor(rgb).to(dev)
        self.mask = torch.as_tensor(mask).float().to(dev)
        self.eraser = torch.as_tensor(eraser).float().to(dev)
        self.target = t.to(dev)

    def forward_only(self, ret_loss=True):
        net = self.net
        n, _, h, w = self.mask.shape
        with torch.no_grad():
            out = net.run(self.mask[:, 0], self.eraser[:, 0], th=0.5,
                          target=self.target.to(torch.uint8).contiguous() if ret_loss else None)
        # softmax(l)[1] > 0.5 is l1 > l0: the argmax over two classes (ties go to class 0 in both)
        comp = out["comp"].unsqueeze(1).float()
        vis = (self.mask > 0).float()
        comp[self.eraser == 0] = vis[self.eraser == 0]
        vis_combo = vis.clone()
        vis_combo[self.eraser == 1] = 0.5
        vis_target = self.target.cpu().clone().float().unsqueeze(1)     # (no 255 "ignore" value gets past set_input)
        ret_tensors = {"common_tensors": [], "mask_tensors": [self.mask, vis_combo, comp, vis_target]}
        if not ret_loss:
            return ret_tensors
        s = out["loss_sums"]
        loss = (self.inmask_weight * s[0] + 1.0 * s[1]) / (n * h * w) / self.world_size
        return ret_tensors, {"loss": loss}

    def step(self):
        """One training step, the reference's in its order (partial_completion_mask.py:116-126): forward on
        cat([mask, eraser]) (no erase, no category scale), the loss over world_size, zero_grad, backward, the gradient
        exchange, the update.  Eager: one launch per node, no graph capture."""
        if self.net.dtype != "fp32":
            raise NotImplementedError("PartialCompletionMask.step: dtype=%r is not in the package (fp32 only; bf16 "
                                      "training of the UNet is not written)." % (self.net.dtype,))
        if getattr(self, "mask", None) is None:
            # the reference's trainer feeds set_input from PartialCompDataset, which is deliberately out of the package
            raise NotImplementedError("PartialCompletionMask.step: no input has been set, and the package has no "
                                      "eraser-synthesising dataset of its own -- self-fed training PCNet-M is not in the "
                                      "package yet; call set_input(rgb, mask, eraser, target) before every step().")
        loss = self.net.loss_train(self.mask, self.eraser, self.target, self.inmask_weight, self.world_size)
        self.optim.zero_grad()
        loss.backward()
        if self.world_size > 1:
            distributed_utils.average_gradients(self.model)
        self.optim.step()
        return {"loss": loss.detach()}
