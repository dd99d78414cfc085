"""Input pipeline with dense masks against run-length masks (instaorder_amd.rle), no network step: BatchPrefetcher over
SupOcclusionOrderBatches on the reader of ``bench.py --host-inputs u8`` (SyntheticReader(500, n_images=32, n_inst=8,
max_side=640, min_side=480, empty_every=0)), B = 256 pairs at S = 256 -- first with the reader as it is, then wrapped in
``rle.RLEReader``, in one process on one GPU.  A third leg repeats the run-length leg with a reader that hands out a
new mask object per item, so that every item uploads its image again as the dense leg does.

Per leg:
  * batches/s: median (and mean) over --batches consumed batches after --warmup (the consumer only waits for each
    batch's event, so this is the rate the pipeline alone sustains: host planning + staging copy + upload + kernels);
  * the bytes one batch uploads, split into images / masks or run tables / descriptors (PairRenderer.last_upload,
    mean over --probe direct batch() calls with the leg's generator state);
  * the time of the decode kernel and of the render kernel per batch from the library's event timing (IoProfScope), taken
    on the probe calls, not on the timed ones (the events cost time of their own).
The first probe batch of all legs must be equal bit for bit, and the masks-or-tables bytes must drop at least 50-fold;
otherwise the exit status is 1.

    python tools/rle_input_bench.py [--batches 20] [--warmup 5] [--B 256] [--S 256] [--out profiles/rle_input_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from instaorder_amd import _lib, datasets, rle, synthetic  # noqa: E402


def make(reader, S, seed=7):
    cfg = dict(input_size=S, patch_or_image="patch", data_mean=[0.485, 0.456, 0.406], data_std=[0.229, 0.224, 0.225],
               load_rgb=True, use_category=False, dataset="InstaOrder", remove_occ_bidirec=0,
               base_aug=dict(flip=True, shift=[-0.2, 0.2], scale=[0.8, 1.2]))
    return datasets.SupOcclusionOrderBatches(cfg, "train", "InstaOrderNet_o", reader, reader.load_image,
                                             rng=np.random.RandomState(seed))


def index_batches(n_img, B, count):
    return [[(s * B + k) % n_img for k in range(B)] for s in range(count)]


class PerItemRLEReader(rle.RLEReader):
    """RLEReader that hands out a new RLEMasks object (same codes) per call, as a dense reader's masks are a new array per
    item: the renderer then places and uploads an image once per item -- separates the effect of the run tables from the
    effect of uploading a shared image once."""

    def get_image_instances(self, idx, *args, **kw):
        out = rle.RLEReader.get_image_instances(self, idx, *args, **kw)
        return (out[0].with_values(out[0].values),) + tuple(out[1:])


def leg(name, reader, a):
    n_img = reader.get_image_length()
    # probe: direct calls on this thread -- bytes, kernel times, and the first batch for the comparison of the legs
    ds = make(reader, a.S)
    L = _lib.lib()
    ups, first = [], None
    L.io_prof_begin_ex(0)
    for idx in index_batches(n_img, a.B, a.probe):
        out = ds.batch(idx)
        ups.append(dict(ds.renderer.last_upload))
        if first is None:
            first = [t.cpu().numpy() for t in out]
    ent = (_lib.ProfEntry * 32)()
    n = L.io_prof_end(ent, 32)
    kern = {e.name.decode(): dict(launches=int(e.launches), ms_per_batch=round(e.total_ms / a.probe, 4),
                                  bytes_per_batch=e.bytes / a.probe) for e in ent[:n]}
    upload = {k: float(np.mean([u[k] for u in ups])) for k in ups[0]}
    # timed: the prefetcher's worker thread and side stream, the consumer only takes the batches
    ds = make(reader, a.S)
    it = datasets.BatchPrefetcher(ds, index_batches(n_img, a.B, a.warmup + a.batches))
    stamps = []
    for k, out in enumerate(it):
        torch.cuda.current_stream().synchronize()
        stamps.append(time.perf_counter())
        del out
    dt = np.diff(stamps[a.warmup - 1:])
    assert len(dt) == a.batches
    # the queue between worker and consumer hands batches over in bursts, so the mean interval is given next to the median
    res = dict(leg=name, batches_per_s=round(1.0 / float(np.median(dt)), 3), batch_ms_median=round(float(np.median(dt)) * 1e3, 2),
               batches_per_s_mean=round(1.0 / float(dt.mean()), 3), batch_ms_mean=round(float(dt.mean()) * 1e3, 2),
               batch_ms_min_max=[round(float(dt.min()) * 1e3, 2), round(float(dt.max()) * 1e3, 2)],
               pairs_per_s=round(a.B / float(np.median(dt)), 1), upload_bytes_per_batch=upload, kernels=kern)
    print(json.dumps(res), flush=True)
    return res, first


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--probe", type=int, default=3)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    assert a.batches >= 1 and a.warmup >= 1 and a.probe >= 1
    _lib.require_gpu()
    torch.cuda.set_device(0)
    rd = synthetic.SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0)
    dense, first_d = leg("dense", rd, a)
    rr = rle.RLEReader(rd)
    runs = [c.size for i in range(rd.get_image_length()) for c in rr.get_image_instances(i)[0].counts]
    rl, first_r = leg("rle", rr, a)
    per_item, first_p = leg("rle, image uploaded per item", PerItemRLEReader(rd), a)
    same = all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(first_d, first_r, first_p))
    ratio = dense["upload_bytes_per_batch"]["masks"] / rl["upload_bytes_per_batch"]["masks"]
    res = dict(tool="tools/rle_input_bench.py", device=torch.cuda.get_device_name(0), csrc_digest=_lib.csrc_digest(),
               B=a.B, S=a.S, batches=a.batches, warmup=a.warmup, probe_batches=a.probe,
               reader="SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0)",
               runs_per_mask=dict(mean=round(float(np.mean(runs)), 1), max=int(np.max(runs))),
               lds_runs=rle.lds_runs(), legs=[dense, rl, per_item], first_batch_equal=bool(same),
               mask_bytes_ratio=round(ratio, 1), rle_over_dense_batches_per_s=round(rl["batches_per_s"] /
                                                                                    dense["batches_per_s"], 3),
               not_measured="a network step next to the pipeline; real COCO / KINS masks; the string parser's cost")
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ok = same and ratio >= 50.0
    if not ok:
        print("FAILED: first batch equal = %s, mask bytes ratio = %.1f (need >= 50)" % (same, ratio))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
