#!/usr/bin/env python3
"""One eager PCNet-M training step (PartialCompletionMask.step) at the recipe's shape: unet2, fp32, batch 32, 256 x 256,
seeded synthetic patches (ellipse masks, as tools/pcnet_bench.py draws them).

Timed: --steps steps (at least 20), each between two device events, after --warmup steps; the median and the spread
(min, max, inter-quartile range) are reported.  Then ONE more step under the library's own per-launch event timing
(io_prof_begin_ex(0)): the time per kernel class, and the launches that touch a full-resolution tensor -- in unet2 the
convolutions at full resolution are exactly those whose real width is 32 (inc, up4), stored at 64: their share of the
step is the cost of the 64-wide layout.  No threshold on time.  A kernel-by-kernel trace is a separate run:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pcnet_train_bench.py --steps 20 --no-classes

    python tools/pcnet_train_bench.py [--batch 32] [--size 256] [--steps 20] [--warmup 3] [--out profiles/pcnet_train_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import instaorder_amd as ia  # noqa: E402
from instaorder_amd import _lib  # noqa: E402


def patches(seed, n, size):
    """n (visible mask, eraser, target) patches: two overlapping ellipses each; the eraser lies over the mask"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    mask, eraser, target = (np.zeros((n, size, size), np.float32) for _ in range(3))
    for i in range(n):
        def ell():
            cy, cx = rng.uniform(0.3 * size, 0.7 * size, 2)
            ry, rx = rng.uniform(0.15 * size, 0.35 * size, 2)
            return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        full, er = ell(), ell()
        mask[i], eraser[i], target[i] = full & ~er, er, full
    return torch.from_numpy(mask)[:, None], torch.from_numpy(eraser)[:, None], torch.from_numpy(target).long()


def model(arch, seed):
    torch.manual_seed(seed)
    m = ia.PartialCompletionMask(dict(algo="PartialCompletionMask", backbone_arch=arch, use_rgb=False, inmask_weight=5.0,
                                      backbone_param=dict(in_channels=2, n_classes=2), optim="SGD", lr=1e-3,
                                      weight_decay=1e-4))
    ia.utils.init_weights(m.net, init_type="kaiming")           # order-1 activations instead of the xavier(0.02) start
    m.switch_to("train")
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arch", default="unet2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-classes", action="store_true", help="skip the per-class step (for a run under a profiler)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20")
    _lib.require_gpu()
    m = model(a.arch, 1)
    mask, eraser, target = patches(2, a.batch, a.size)
    m.set_input(rgb=None, mask=mask, eraser=eraser, target=target)
    losses = [float(m.step()["loss"]) for _ in range(a.warmup)]
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    for e0, e1 in ev:
        e0.record()
        out = m.step()
        e1.record()
    torch.cuda.synchronize()
    losses.append(float(out["loss"]))
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    q = statistics.quantiles(ms, n=4)
    res = dict(workload="pcnet_m eager training step", arch=a.arch, dtype="fp32", batch=a.batch, size=a.size, steps=a.steps,
               warmup=a.warmup, step_ms_median=round(statistics.median(ms), 3), step_ms_min=round(ms[0], 3),
               step_ms_max=round(ms[-1], 3), step_ms_iqr=round(q[2] - q[0], 3),
               patches_per_s=round(1e3 * a.batch / statistics.median(ms), 1), loss_first=round(losses[0], 6),
               loss_last=round(losses[-1], 6), peak_memory_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
               csrc=_lib.csrc_digest())
    if not a.no_classes:
        L = _lib.lib()
        L.io_prof_begin_ex(0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.step()
        e1.record()
        torch.cuda.synchronize()
        ent = (_lib.ProfEntry * 4096)()
        n = L.io_prof_launches(ent, 4096)
        launches = [(e.name.decode(), e.total_ms, e.bytes, e.flops) for e in ent[:n]]
        L.io_prof_end((_lib.ProfEntry * 64)(), 64)
        wall = e0.elapsed_time(e1)
        classes = {}
        for name, t, _, _ in launches:
            c = classes.setdefault(name, [0, 0.0])
            c[0] += 1
            c[1] += t
        px = float(a.batch) * a.size * a.size
        full = {}
        for name, t, b, f in launches:
            if f >= 0.99 * 2.0 * px * 9 * 64 * 64 and b >= 0.99 * 4.0 * px * 128:      # a 3x3 convolution pass at full resolution
                c = full.setdefault(name, [0, 0.0])
                c[0] += 1
                c[1] += t
        full_ms = sum(v[1] for v in full.values())
        res.update(profiled_step_ms=round(wall, 3), library_ms=round(sum(v[1] for v in classes.values()), 3),
                   classes_ms={k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in sorted(classes.items())},
                   full_resolution_conv_ms={k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in sorted(full.items())},
                   full_resolution_conv_share=round(full_ms / wall, 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
