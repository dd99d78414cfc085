"""Host cost of the annotation readers (instaorder_amd.readers): ``get_image_instances`` per image and a
``SupOcclusionOrderBatches.plan`` loop, for ``masks="dense"`` against ``masks="encoded"`` (cold: the first visit of an
image; cached: a later one).  The annotation file is written from a seed in COCO's form: --images images of 640 x 480 with
5-40 polygon instances of 10-60 vertices each, InstaOrder-style occlusion and depth entries over random pairs.

The dense leg is what the reference's reader does on every call -- rasterise every instance of the image on the host -- with
one caveat: its rasteriser here is ``PolyMasks.to_dense()`` in NumPy, not pycocotools' C code, which is not available to
measure.  So the dense figure is an upper bound on the reference's host cost, and the figure to read is the absolute time
of the encoded legs.  No ratio is asserted, nothing is held to a threshold.

The host part needs no GPU.  ``--gpu`` adds the device leg of ``COCOAReader``: per image, the masks decoded on the device
(``to_device``) and ``readers.mask_bboxes`` on them, timed with events (kernels only) and by the clock (with the copy back).

    python tools/reader_bench.py [--images 200] [--items 400] [--seed 7] [--gpu] [--out profiles/reader_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instaorder_amd import datasets, readers  # noqa: E402

W, H = 640, 480


def write_annotations(directory, seed, n_images):
    """instaorder_val2017.json + instances_val2017.json under ``directory``; returns the order file's name"""
    rs = np.random.RandomState(seed)
    images, anns, order = [], [], []
    aid = 1
    for k in range(n_images):
        images.append(dict(id=1000 + k, file_name="%012d.jpg" % (1000 + k), width=W, height=H))
        n = int(rs.randint(5, 41))
        ids = []
        for _ in range(n):
            verts = int(rs.randint(10, 61))
            w, h = rs.uniform(30, 320), rs.uniform(30, 240)
            cx, cy = rs.uniform(w / 2, W - w / 2), rs.uniform(h / 2, H - h / 2)
            t = np.linspace(0.0, 2 * np.pi, verts, endpoint=False)
            r = rs.uniform(0.7, 1.0, verts)
            ring = np.stack([cx + r * w / 2 * np.cos(t), cy + r * h / 2 * np.sin(t)], axis=1)
            flat = np.round(ring, 2).reshape(-1).tolist()
            anns.append(dict(id=aid, image_id=1000 + k, category_id=int(rs.randint(1, 91)), iscrowd=0, segmentation=[flat],
                             bbox=[round(cx - w / 2, 2), round(cy - h / 2, 2), round(w, 2), round(h, 2)], area=round(w * h, 1)))
            ids.append(aid)
            aid += 1
        occ, depth = [], []
        for _ in range(2 * n):
            i, j = (int(v) for v in rs.choice(n, 2, replace=False))
            u = rs.rand()
            occ.append(dict(order="%d<%d" % (i, j) if u < 0.85 else "%d<%d & %d<%d" % (i, j, j, i)))
            depth.append(dict(order="%d%s%d" % (i, "=" if rs.rand() < 0.15 else "<", j), overlap=bool(rs.rand() < 0.5),
                              count=int(rs.randint(1, 4))))
        order.append(dict(image_id=1000 + k, instance_ids=ids, occlusion=occ, depth=depth))
    with open(os.path.join(directory, "instances_val2017.json"), "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[]), f)
    fn = os.path.join(directory, "instaorder_val2017.json")
    with open(fn, "w") as f:
        json.dump(dict(annotations=order), f)
    return fn, len(anns), sum(len(a["segmentation"][0]) // 2 for a in anns)


def per_image_ms(rd, n):
    t = []
    for i in range(n):
        t0 = time.perf_counter()
        rd.get_image_instances(i, with_gt=True)
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.asarray(t)
    return dict(mean_ms=round(float(t.mean()), 4), median_ms=round(float(np.median(t)), 4), max_ms=round(float(t.max()), 4))


def plan_loop_ms(rd, items, seed):
    cfg = dict(input_size=256, patch_or_image="patch", data_mean=[0.485, 0.456, 0.406], data_std=[0.229, 0.224, 0.225],
               load_rgb=True, use_category=False, dataset="InstaOrder", remove_occ_bidirec=0,
               base_aug=dict(flip=True, shift=[-0.2, 0.2], scale=[0.8, 1.2]))
    ds = datasets.SupOcclusionOrderBatches(cfg, "train", "InstaOrderNet_o", rd, None, rng=np.random.RandomState(seed))
    idx = np.random.RandomState(seed + 1).randint(0, len(ds), items)
    t0 = time.perf_counter()
    plans = [ds.plan(int(i)) for i in idx]
    ms = (time.perf_counter() - t0) * 1e3 / items
    return round(ms, 4), [(p["idx1"], p["idx2"], p["box"], p["flip"], tuple(int(v) for v in p["target"])) for p in plans]


def gpu_leg(rd, n):
    import torch
    from instaorder_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    ev, wall, pixels = [], [], 0
    for rep in range(2):                                              # the first pass warms the allocator and the library
        ev, wall, pixels = [], [], 0
        for i in range(n):
            t = rd.get_image_instances(i)[0].to_device("cuda")
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            out = torch.empty((t.shape[0], 5), dtype=torch.int32, device="cuda")
            a.record()
            _lib.check(_lib.lib().io_mask_bbox_u8(t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], 1, out.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream), "io_mask_bbox_u8")
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
            t0 = time.perf_counter()
            got = readers.mask_bboxes(t)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(got, out.cpu().numpy())
            pixels += t.numel()
    return dict(device=torch.cuda.get_device_name(0), images=n, kernels_ms_per_image=round(float(np.mean(ev)), 4),
                call_with_copy_ms_per_image=round(float(np.mean(wall)), 4),
                mask_bytes_per_image=int(pixels // n), csrc_digest=_lib.csrc_digest())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--items", type=int, default=400)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--gpu-images", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as d:
        fn, n_inst, n_verts = write_annotations(d, a.seed, a.images)
        t0 = time.perf_counter()
        dense = readers.InstaOrderReader(fn, masks="dense", cache_images=a.images)
        load_ms = (time.perf_counter() - t0) * 1e3
        enc = readers.InstaOrderReader(fn, masks="encoded", cache_images=a.images)
        res = dict(tool="tools/reader_bench.py", images=a.images, instances=n_inst, vertices=n_verts, size=[H, W],
                   items=a.items, seed=a.seed, open_both_files_ms=round(load_ms, 1),
                   get_image_instances=dict(dense=per_image_ms(dense, a.images), encoded_cold=per_image_ms(enc, a.images),
                                            encoded_cached=per_image_ms(enc, a.images)))
        d_ms, d_plans = plan_loop_ms(dense, a.items, a.seed)
        e_ms, e_plans = plan_loop_ms(enc, a.items, a.seed)
        res["plan_ms_per_item"] = dict(dense=d_ms, encoded_cached=e_ms)
        res["plans_equal"] = d_plans == e_plans
        res["caveat"] = ("dense rasterises with PolyMasks.to_dense() in NumPy, not pycocotools' C code: an upper bound on the "
                         "reference's host cost")
        res["gpu"] = gpu_leg(enc, min(a.gpu_images, a.images)) if a.gpu else "not measured"
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0 if res["plans_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
