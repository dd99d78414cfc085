"""Input pipeline with polygon masks (instaorder_amd.poly) against the same masks as dense arrays, no network step: the
legs of tools/rle_input_bench.py (BatchPrefetcher over SupOcclusionOrderBatches, the reader of ``bench.py --host-inputs
u8``, B = 256 pairs at S = 256, one process on one GPU) with every instance mask replaced by a polygon of --verts vertices
around its box.  The dense leg's masks are those polygons rasterised before the timing starts, so they cost its host
nothing: the figure shows whether the polygon path keeps up with free dense masks, not what it saves over a host
rasteriser (pycocotools is not measured here).

A third leg repeats the polygon leg with a new mask object per item, so that every item uploads its image again as the
dense leg does.  Per leg: batches/s, the bytes one batch uploads and the kernel times per batch, as in
tools/rle_input_bench.py.  The first probe batch of all legs must be equal bit for bit; otherwise the exit status is 1.
No threshold on time or bytes.

    python tools/poly_input_bench.py [--batches 20] [--warmup 5] [--B 256] [--S 256] [--verts 36] [--out profiles/poly_input_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rle_input_bench as base  # noqa: E402  (puts the repository root on sys.path)
from instaorder_amd import _lib, poly, synthetic  # noqa: E402


class PolygonReader(object):
    """The wrapped reader with each instance mask replaced by one polygon of ``verts`` vertices: a ring around the
    instance's box with a jittered radius, coordinates to two decimals as annotations carry them.  ``dense=True`` hands
    out the same masks rasterised (``to_dense()``, once per image, at construction).  ``per_item=True`` hands out a new
    PolyMasks object (same vertices) per call, as a dense reader's masks are a new array per item: the renderer then
    uploads an image once per item, which separates the effect of the vertices from that of sharing an image."""

    def __init__(self, reader, verts, dense, per_item=False):
        self._reader, self._dense, self._per_item, self._masks = reader, dense, per_item, []
        for i in range(reader.get_image_length()):
            modal, _, bboxes = reader.get_image_instances(i, with_gt=True)[:3]
            n, H, W = modal.shape
            rs = np.random.RandomState(1000 + i)
            inst = []
            for x, y, w, h in np.asarray(bboxes, dtype=np.float64):
                t = np.linspace(0.0, 2 * np.pi, verts, endpoint=False)
                r = rs.uniform(0.45, 0.65, verts)
                ring = np.stack([x + w / 2 + r * w * np.cos(t), y + h / 2 + r * h * np.sin(t)], axis=1)
                inst.append([np.round(ring, 2).reshape(-1).tolist()])
            pm = poly.PolyMasks(inst, H, W)
            self._masks.append(pm.to_dense() if dense else pm)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._reader, name)

    def get_image_instances(self, idx, *args, **kw):
        out = self._reader.get_image_instances(idx, *args, **kw)
        m = self._masks[int(idx)]
        if self._dense:
            m = m.copy()                                               # a dense reader's masks are a new array per item
        elif self._per_item:
            m = m.with_values(m.values)
        return (m,) + tuple(out[1:])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--probe", type=int, default=3)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--verts", type=int, default=36)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    assert a.batches >= 1 and a.warmup >= 1 and a.probe >= 1 and a.verts >= 3
    _lib.require_gpu()
    torch.cuda.set_device(0)
    rd = synthetic.SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0)
    dense, first_d = base.leg("dense (the polygons rasterised beforehand)", PolygonReader(rd, a.verts, True), a)
    pol, first_p = base.leg("polygons", PolygonReader(rd, a.verts, False), a)
    per_item, first_i = base.leg("polygons, image uploaded per item", PolygonReader(rd, a.verts, False, per_item=True), a)
    same = all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(first_d, first_p, first_i))
    ratio = dense["upload_bytes_per_batch"]["masks"] / pol["upload_bytes_per_batch"]["masks"]
    res = dict(tool="tools/poly_input_bench.py", device=torch.cuda.get_device_name(0), csrc_digest=_lib.csrc_digest(),
               B=a.B, S=a.S, batches=a.batches, warmup=a.warmup, probe_batches=a.probe, verts_per_polygon=a.verts,
               reader="SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0), masks "
                      "replaced by polygons",
               scan_words=poly.scan_words(), legs=[dense, pol, per_item], first_batch_equal=bool(same),
               mask_bytes_ratio=round(ratio, 1),
               polygons_over_dense_batches_per_s=round(pol["batches_per_s"] / dense["batches_per_s"], 3),
               per_item_polygons_over_dense_batches_per_s=round(per_item["batches_per_s"] / dense["batches_per_s"], 3),
               not_measured="the host rasteriser (pycocotools) the polygon path replaces: the dense leg's masks are free; a "
                            "network step next to the pipeline; real COCO polygons")
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not same:
        print("FAILED: the first batch of the legs differs")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
