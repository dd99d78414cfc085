#!/usr/bin/env python3
"""optim: Adam on one MI355X -- the fused update against torch.optim.Adam (default, multi-tensor) and the MiDaS training
step with each.  Device-event medians over warmed iterations; prints one JSON line.

  (a) update of ResNet-50's flat buffer (23.5 M floats): io_adam_step vs torch.optim.Adam over the 161 strided views
  (b) update of InstaDepthNet_od's 680 parameters: FlatAdam.step(gathered=True) vs torch.optim.Adam
  (c) InstaDepthNet_od training step, bf16, 384^2, 16 pairs (BASELINE configs[4]) with optim: Adam: torch.optim.Adam
      (eager per-tensor path) vs FlatAdam (flat buffer, WeightPlan, hipGraph)
  (d) --clip: gradient clipping on both flat buffers, momentum SGD and Adam: the fused clipped step (io_grad_norm + the
      clipped update) vs torch.nn.utils.clip_grad_norm_ over the parameter views followed by the plain fused step vs the
      plain fused step alone
usage: python tools/optim_bench.py [--iters 100] [--warmup 10] [--step-iters 10] [--skip-step] [--clip]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_TBS = 6.3     # achievable HBM rate assumed for the bound (not measured here)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def update_bench(args):
    from instaorder_amd import resnet_cls
    from instaorder_amd.optim import FlatAdam, FusedAdam
    out = {}
    net = resnet_cls.resnet50_cls(in_channels=5, num_classes=[2, 3]).cuda()
    net.flat_grads.normal_()
    net.attach_grads()
    n = net.flat_params.numel()
    fused = FusedAdam(net, lr=1e-7, betas=(0.9, 0.999))
    ref = torch.optim.Adam(list(net.parameters()), lr=1e-7, betas=(0.9, 0.999))
    f_ms = timed(fused.step, args.iters, args.warmup)
    t_ms = timed(ref.step, args.iters, args.warmup)
    bound = 28.0 * n / (HBM_TBS * 1e12) * 1e3
    out["resnet50"] = dict(floats=n, tensors=len(fused._params), fused_ms=round(f_ms, 4), torch_adam_ms=round(t_ms, 4),
                           speedup=round(t_ms / f_ms, 2), bound_ms_at_6p3TBs=round(bound, 4),
                           share_of_bound=round(bound / f_ms, 3), achieved_TBs=round(28.0 * n / (f_ms * 1e-3) / 1e12, 2))
    del net, fused, ref
    from instaorder_amd import midas_net
    torch.manual_seed(0)
    mod = midas_net.InstaDepthNet_od(None, non_negative=True).cuda()
    flat = FlatAdam(mod, lr=1e-9, betas=(0.9, 0.999))
    flat.flat_grads.normal_()
    for p, (off, k) in zip(flat._params, flat._spans):
        p.grad = flat.flat_grads[off:off + k].view(p.shape)
    ref = torch.optim.Adam(flat._params, lr=1e-9, betas=(0.9, 0.999))
    f_ms = timed(lambda: flat.step(gathered=True), args.iters, args.warmup)
    t_ms = timed(ref.step, args.iters, args.warmup)
    n = flat.flat_params.numel()
    bound = 28.0 * n / (HBM_TBS * 1e12) * 1e3
    out["instadepthnet_od"] = dict(floats=n, tensors=len(flat._params), fused_ms=round(f_ms, 4),
                                   torch_adam_ms=round(t_ms, 4), speedup=round(t_ms / f_ms, 2),
                                   bound_ms_at_6p3TBs=round(bound, 4), share_of_bound=round(bound / f_ms, 3))
    return out


def clip_bench(args):
    """Per flat buffer and optimiser: (a) fused clipped step, (b) clip_grad_norm_ over the views + the plain fused step,
    (c) the plain fused step.  max_grad_norm 1.0 is far below the norm of the random gradients, so (a) and (b) scale."""
    from instaorder_amd import midas_net, resnet_cls
    from instaorder_amd.optim import FlatAdam, FlatSGD, FusedAdam, FusedSGD
    out = {}

    def rows(opt, step, params, n, bytes_per_float):
        def torch_then_fused():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            step()
        opt.max_grad_norm = None
        plain = timed(step, args.iters, args.warmup)
        both = timed(torch_then_fused, args.iters, args.warmup)
        opt.max_grad_norm = 1.0
        fused = timed(step, args.iters, args.warmup)
        stats = opt.grad_stats()
        assert stats["steps"] == args.iters + args.warmup and stats["skipped"] == 0
        return dict(floats=n, fused_clipped_ms=round(fused, 4), torch_clip_plus_fused_ms=round(both, 4),
                    unclipped_ms=round(plain, 4), extra_ms=round(fused - plain, 4),
                    speedup_vs_torch_clip=round(both / fused, 2),
                    clipped_TBs=round((bytes_per_float + 4.0) * n / (fused * 1e-3) / 1e12, 2))

    net = resnet_cls.resnet50_cls(in_channels=5, num_classes=[2, 3]).cuda()
    net.flat_grads.normal_()
    net.attach_grads()
    params = list(net.parameters())
    n = net.flat_params.numel()
    for name, opt, bpf in (("sgd", FusedSGD(net, lr=1e-9, momentum=0.9, weight_decay=1e-4), 20.0),
                           ("adam", FusedAdam(net, lr=1e-9, betas=(0.9, 0.999)), 28.0)):
        out["resnet50_" + name] = rows(opt, opt.step, params, n, bpf)
    del net, opt, params
    for name, cls, kw, bpf in (("sgd", FlatSGD, dict(momentum=0.9, weight_decay=1e-4), 20.0),
                               ("adam", FlatAdam, dict(betas=(0.9, 0.999)), 28.0)):
        torch.manual_seed(0)
        mod = midas_net.InstaDepthNet_od(None, non_negative=True).cuda()
        opt = cls(mod, lr=1e-9, **kw)
        opt.flat_grads.normal_()
        for p, (off, k) in zip(opt._params, opt._spans):
            p.grad = opt.flat_grads[off:off + k].view(p.shape)
        out["instadepthnet_od_" + name] = rows(opt, lambda: opt.step(gathered=True), opt._params, opt.flat_params.numel(),
                                               bpf)
        del mod, opt
        torch.cuda.empty_cache()
    return out


def step_bench(args):
    import instaorder_amd as ia
    from instaorder_amd import synthetic
    B, S = 16, 384
    batch = synthetic.make_depth_batch(1000, B, S)
    t = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    res = {}
    for form in ("torch_adam_eager", "flat_adam_graph"):
        torch.manual_seed(0)
        cfg = dict(algo="InstaDepthNet_od", lr=1e-5, weight_decay=1e-4, optim="Adam", beta1=0.9, pretrained_weight=None,
                   use_rgb=True, dtype="bf16", overlap_weight=0.0, distinct_weight=0.0, dorder_weight=1.0,
                   smooth_weight=0.1, occ_order_weight=0.0)
        m = ia.InstaDepthNet_od(cfg, dist_model=False)
        if form == "torch_adam_eager":
            m.optim = torch.optim.Adam(m.model.parameters(), lr=1e-5, betas=(0.9, 0.999))
        m.switch_to("train")
        m.set_input(t["rgb"], t["modal1"], t["modal2"], t["depth_order"], t["count"], t["is_overlap"], t["occ_order"])
        ms = timed(m.step, args.step_iters, 3)
        res[form] = dict(step_ms=round(ms, 3), pairs_per_s=round(B / (ms * 1e-3), 1),
                         graph=m._graph is not None, weight_plan=bool(m._wplan))
        del m
        torch.cuda.empty_cache()
    res["speedup"] = round(res["torch_adam_eager"]["step_ms"] / res["flat_adam_graph"]["step_ms"], 3)
    return dict(shape="InstaDepthNet_od bf16 384^2 x 16 pairs", **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--clip", action="store_true", help="only the gradient-clipping rows (d)")
    args = ap.parse_args()
    from instaorder_amd import _lib
    _lib.require_gpu()
    if args.clip:
        print(json.dumps(dict(bench="optim_clip", csrc=_lib.csrc_digest(), iters=args.iters, clip=clip_bench(args))))
        return
    out = dict(bench="optim_adam", csrc=_lib.csrc_digest(), update=update_bench(args))
    if not args.skip_step:
        out["train_step"] = step_bench(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
