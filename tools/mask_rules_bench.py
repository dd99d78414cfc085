"""Host vs device time per image of the mask-based order rules (instaorder_amd.mask_rules against the host loops of
instaorder_amd.inference) on seeded synthetic scenes: n = 10 / 20 / 40 instances at 640x480 and 1242x375, for the
midas_pretrained disparity selection ('median' / 'mean', all pairs), the 'nbor' pair selection and infer_gt_order.

Each row: the host time of one call (after a warm-up call), the median device time over --reps synchronised calls (after
a warm-up), and the check that both gave the same result -- a row whose outputs differ is reported as a failure, not
timed.  The device timings include the mask upload / validation and the single copy back, as a caller sees them; the
host timings of the disparity selection include the copy of the device masks to the host that inference.py does.

    python tools/mask_rules_bench.py [--sizes 640x480,1242x375] [--ns 10,20,40] [--reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instaorder_amd import _lib, inference, mask_rules  # noqa: E402


def scene(seed, n, H, W):
    """SyntheticReader-style instances (rectangles and ellipses, 5-30 % of the shorter side), an amodal mask that extends
    each instance, and a smooth positive disparity map"""
    rs = np.random.RandomState(seed)
    modal = np.zeros((n, H, W), np.uint8)
    amodal = np.zeros((n, H, W), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    s = min(H, W)
    for i in range(n):
        h, w = rs.randint(s // 20, s * 3 // 10), rs.randint(s // 20, s * 3 // 10)
        top, left = rs.randint(0, H - h), rs.randint(0, W - w)
        if i % 2:
            modal[i, top:top + h, left:left + w] = 1
        else:
            cy, cx = top + h / 2.0, left + w / 2.0
            modal[i][((yy - cy) / (h / 2.0)) ** 2 + ((xx - cx) / (w / 2.0)) ** 2 <= 1.0] = 1
        amodal[i, max(top - 4, 0):top + h + 4, max(left - 4, 0):left + w + 4] = 1
    disp = (0.2 + np.sin(yy / 37.0) ** 2 + 0.5 * np.cos(xx / 53.0) ** 2 + 0.05 * rs.rand(H, W)).astype(np.float32)
    return modal, amodal, disp


def host_midas(disp, masks_dev, pairs, method):
    """the loop of inference.infer_order_sup_depth (midas_pretrained) over the pairs"""
    masks_np = masks_dev.cpu().numpy()
    n = masks_np.shape[0]
    order = np.zeros((n, n), dtype=np.int64)
    for i, j in pairs:
        a = inference.net_forward_midas_pretrained(disp, masks_np[i], masks_np[j], method)
        order[i, j], order[j, i] = {0: (1, 0), 1: (0, 1), 2: (2, 2)}[a]
    return order


def timed(fn, reps):
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1242x375")
    ap.add_argument("--ns", default="10,20,40")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows, failed = [], 0
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for n in (int(v) for v in a.ns.split(",")):
            modal, amodal, disp_np = scene(1000 * n + W, n, H, W)
            disp = torch.from_numpy(disp_np).to(dev)
            masks_dev = torch.from_numpy(modal).to(dev).float()         # the 'resize' / 'orig' form: float, on the device
            pairs = inference.upper_pairs(n)
            cases = [
                ("midas_median", lambda: host_midas(disp, masks_dev, pairs, "median"),
                 lambda: mask_rules.depth_orders_from_disp(disp, masks_dev, pairs, "median")),
                ("midas_mean", lambda: host_midas(disp, masks_dev, pairs, "mean"),
                 lambda: mask_rules.depth_orders_from_disp(disp, masks_dev, pairs, "mean")),
                ("nbor", lambda: inference.select_pairs(modal, "nbor"), lambda: mask_rules.select_pairs(modal, "nbor")),
                ("gt_order", lambda: inference.infer_gt_order(modal, amodal),
                 lambda: mask_rules.infer_gt_order(modal, amodal)),
            ]
            for name, host, device in cases:
                timed(host, 1)
                h_out, h_t = timed(host, 1)
                timed(device, 1)
                d_out, d_t = timed(device, a.reps)
                same = (h_out == d_out) if isinstance(h_out, list) else bool(np.array_equal(h_out, d_out))
                row = dict(rule=name, W=W, H=H, n=n, pairs=len(pairs), same=same,
                           host_ms=round(h_t * 1e3, 3) if same else None, device_ms=round(d_t * 1e3, 3) if same else None,
                           speedup=round(h_t / d_t, 1) if same else None)
                failed += not same
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("%-13s %9s %4s %10s %10s %8s" % ("rule", "size", "n", "host ms", "device ms", "x"))
    for r in rows:
        if r["same"]:
            print("%-13s %9s %4d %10.2f %10.3f %8.1f" % (r["rule"], "%dx%d" % (r["W"], r["H"]), r["n"], r["host_ms"],
                                                          r["device_ms"], r["speedup"]))
        else:
            print("%-13s %9s %4d   OUTPUTS DIFFER" % (r["rule"], "%dx%d" % (r["W"], r["H"]), r["n"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(gpu=torch.cuda.get_device_name(0), reps=a.reps, rows=rows), f, indent=1)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
