"""PCNet-M order recovery (``inference.infer_order``) at the Tester's setting -- unet2, 256 x 256 patches, pairs='all',
fp32 -- for images with 8 and 16 instances (56 and 240 ordered patches), with the 32-channel convolution kernel on and
off (``unet.set_co32``; off = those layers through the dense launcher with their outputs padded to 64 channels).

The two routes alternate on the same box in one process: --warmup calls each, then --repeats timed calls each (wall time
around a device synchronise), reported as medians with the spread.  One more call per route runs under the library's
event timing (io_prof_begin_ex(0)) and gives the time per kernel class: the UNet's share of the call (all convolution
classes + pooling / upsample-concat / pack / head) and the share of the 32-channel kernel.  The order matrices of the two
routes must be equal; otherwise the exit status is 1.  No threshold on time: a route that is slower is reported as it is.

    python tools/pcnet_bench.py [--instances 8 16] [--repeats 7] [--warmup 2] [--out profiles/pcnet_infer_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import instaorder_amd as ia  # noqa: E402
from instaorder_amd import _lib, evaluate, inference, unet  # noqa: E402

H, W = 480, 640
CONV_CLASSES = ("conv_nt_kernel<128,false>", "conv_nt_kernel<64,false>", "conv_nt_kernel<64,true>", "conv_nt_kernel<wino>")


def scene(seed, n):
    """n overlapping ellipses, each drawn over the earlier ones (visible masks), and their tight boxes; the first seed
    from ``seed`` on that leaves every instance visible"""
    while True:
        sc = _scene(seed, n)
        if len(sc[0]) == n:
            return sc
        seed += 1000


def _scene(seed, n):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    owner = np.full((H, W), -1)
    for i in range(n):
        cy, cx = rng.uniform(0.25 * H, 0.75 * H), rng.uniform(0.2 * W, 0.8 * W)
        ry, rx = rng.uniform(40, 110), rng.uniform(40, 110)
        owner[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = i
    keep = [i for i in range(n) if (owner == i).any()]
    modal = np.stack([(owner == i).astype(np.uint8) for i in keep])
    boxes = []
    for m in modal:
        ys, xs = np.where(m > 0)
        boxes.append([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1])
    return modal, np.ones(len(keep), np.int64), evaluate.expand_bbox(boxes, 3.0)


def model(seed):
    torch.manual_seed(seed)
    m = ia.PartialCompletionMask(dict(algo="PartialCompletionMask", backbone_arch="unet2", use_rgb=False, inmask_weight=5.0,
                                      backbone_param=dict(in_channels=2, n_classes=2), optim="SGD", lr=1e-3,
                                      weight_decay=1e-4))
    ia.utils.init_weights(m.net, init_type="kaiming")           # order-1 activations instead of the xavier(0.02) start
    m.switch_to("eval")
    return m


def call(m, sc):
    t = time.perf_counter()
    order = inference.infer_order(m, None, sc[0], sc[1], sc[2], "all", th=0.5, input_size=256, min_input_size=16)
    torch.cuda.synchronize()
    return time.perf_counter() - t, order


def profiled(m, sc):
    L = _lib.lib()
    L.io_prof_begin_ex(0)
    wall, _ = call(m, sc)
    ent = (_lib.ProfEntry * 64)()
    n = L.io_prof_end(ent, 64)
    ms = {e.name.decode(): e.total_ms for e in ent[:n]}
    co32 = ms.get("conv3x3_co32", 0.0)
    net = co32 + ms.get("unet_misc", 0.0) + sum(ms.get(k, 0.0) for k in CONV_CLASSES)
    return dict(call_ms=round(1e3 * wall, 3), unet_ms=round(net, 3), unet_share=round(net / (1e3 * wall), 4),
                co32_ms=round(co32, 3), co32_share=round(co32 / (1e3 * wall), 4),
                classes_ms={k: round(v, 3) for k, v in sorted(ms.items())})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--instances", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    _lib.require_gpu()
    m = model(3)
    prev = unet.get_co32()
    rows, same = [], True
    try:
        for n in a.instances:
            sc = scene(100 + n, n)
            patches = len(sc[0]) * (len(sc[0]) - 1)
            times, orders = {True: [], False: []}, {}
            for it in range(a.warmup + a.repeats):
                for on in (True, False):                       # the two routes alternate
                    unet.set_co32(on)
                    t, orders[on] = call(m, sc)
                    if it >= a.warmup:
                        times[on].append(t)
            same = same and bool(np.array_equal(orders[True], orders[False]))
            row = dict(instances=len(sc[0]), patches=patches, input_size=256, net="unet2", repeats=a.repeats, warmup=a.warmup,
                       orders_equal=bool(np.array_equal(orders[True], orders[False])))
            for on, name in ((True, "co32"), (False, "padded64")):
                unet.set_co32(on)
                ts = sorted(times[on])
                med = statistics.median(ts)
                row[name] = dict(median_ms=round(1e3 * med, 3), min_ms=round(1e3 * ts[0], 3), max_ms=round(1e3 * ts[-1], 3),
                                 patches_per_s=round(patches / med, 1), profiled=profiled(m, sc))
            row["co32_speedup"] = round(row["padded64"]["median_ms"] / row["co32"]["median_ms"], 4)
            rows.append(row)
            print(json.dumps(row))
    finally:
        unet.set_co32(prev)
    out = dict(tool="tools/pcnet_bench.py", device=torch.cuda.get_device_name(0), csrc_digest=_lib.csrc_digest(), rows=rows)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
