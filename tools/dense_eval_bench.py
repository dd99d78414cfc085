#!/usr/bin/env python3
"""Dense-disparity evaluation throughput at the KITTI input shape (352 x 1216): MidasNet forward + the device metrics
(io_depth_errors_median) for B = 1, 4, 8 in fp32 and bf16, against the reference's per-image pattern on the same forward
(.cpu() of each disparity map, then the 'median' conversion and compute_errors in NumPy on the host).

Forward and metrics are timed separately with device events; the host pattern with a wall clock after a synchronise.
Seeded weights and inputs (no dataset, no image decode: the reader / render path is not in these numbers).

    python tools/dense_eval_bench.py [--iters 5] [--warmup 2] [--out profiles/dense_eval_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_metrics(disp, gt_raw, min_depth=1e-3, max_depth=80.0):
    """the reference's per-image host arithmetic (NumPy fp32, as test_disp_KITTI.py does it)"""
    gt = gt_raw.astype(np.float32) / 256.0
    norm = (disp - disp.min()) / disp.max()
    depth = 1 / (norm + 1e-3)
    valid = (gt >= min_depth) & (gt <= max_depth)
    depth *= np.median(gt[valid]) / np.median(depth[valid])
    depth[depth < min_depth] = min_depth
    depth[depth > max_depth] = max_depth
    g, p = gt[valid], depth[valid]
    thr = np.maximum(g / p, p / g)
    d = np.log(p) - np.log(g)
    return ((np.abs(g - p) / g).mean(), (((g - p) ** 2) / g).mean(), np.sqrt(((g - p) ** 2).mean()),
            np.sqrt(((np.log(g) - np.log(p)) ** 2).mean()), (thr < 1.25).mean(), (thr < 1.25 ** 2).mean(),
            (thr < 1.25 ** 3).mean(), np.sqrt((d ** 2).mean() - d.mean() ** 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from instaorder_amd import _lib, dense_eval, midas_net, synthetic
    _lib.require_gpu()
    torch.cuda.set_device(0)
    net = midas_net.MidasNet(non_negative=True).cuda()
    sd = net.state_dict()
    vals = synthetic.make_spec_state_dict(61, [(k, tuple(v.shape), None) for k, v in sd.items()])
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in vals.items()}, strict=True)
    net.eval()
    H, W = dense_eval.KITTI_H, dense_eval.KITTI_W
    rs = np.random.RandomState(62)
    results = []
    for dtype in args.dtypes.split(","):
        net.dtype = dtype
        for B in [int(b) for b in args.batches.split(",")]:
            img = torch.from_numpy(rs.standard_normal((B, 3, H, W)).astype(np.float32)).cuda()
            gt_np = np.stack([synthetic.sparse_gt_u16(rs, H, W) for _ in range(B)])
            gt = torch.from_numpy(gt_np.view(np.int16)).cuda()
            out = torch.empty((B, dense_eval.ROW_WIDTH), dtype=torch.float64, device="cuda")
            fwd_ms, met_ms, host_ms = [], [], []
            for it in range(args.warmup + args.iters):
                e0, e1, e2 = torch.cuda.Event(True), torch.cuda.Event(True), torch.cuda.Event(True)
                e0.record()
                with torch.no_grad():
                    disp = net._encode_decode(img)[0].reshape(B, H, W)
                e1.record()
                dense_eval.depth_errors_median(disp, gt, out=out)
                e2.record()
                rows = out.cpu()                              # the one read-back of a run
                t0 = time.perf_counter()
                for b in range(B):                            # the reference: per image .cpu() + NumPy
                    host_metrics(disp[b].cpu().numpy(), gt_np[b])
                t1 = time.perf_counter()
                if it >= args.warmup:
                    fwd_ms.append(e0.elapsed_time(e1))
                    met_ms.append(e1.elapsed_time(e2))
                    host_ms.append((t1 - t0) * 1e3)
            assert torch.isfinite(rows[:, :8]).all() or not torch.isfinite(disp).all()
            f, m, h = float(np.median(fwd_ms)), float(np.median(met_ms)), float(np.median(host_ms))
            r = dict(dtype=dtype, B=B, forward_ms=round(f, 3), metrics_ms=round(m, 4), host_metrics_ms=round(h, 3),
                     images_per_s=round(B / ((f + m) / 1e3), 2), ref_pattern_images_per_s=round(B / ((f + h) / 1e3), 2),
                     metrics_ms_per_image=round(m / B, 4), host_metrics_ms_per_image=round(h / B, 3),
                     forward_ms_min_max=[round(min(fwd_ms), 3), round(max(fwd_ms), 3)],
                     metrics_ms_min_max=[round(min(met_ms), 4), round(max(met_ms), 4)])
            print(json.dumps(r), flush=True)
            results.append(r)
    doc = dict(tool="tools/dense_eval_bench.py", command=" ".join(["python"] + sys.argv), shape=[H, W],
               iters=args.iters, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               csrc_digest=_lib.csrc_digest(), results=results,
               not_measured="image decode / render and the reader thread; multi-GPU sharding; accuracy on real KITTI / DIW")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(doc, fh, indent=1)
    return doc


if __name__ == "__main__":
    main()
