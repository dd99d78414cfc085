#!/usr/bin/env python3
"""Generate tests/golden/readers.npz by running the REAL reference readers (datasets/reader.py: InstaOrderDataset,
COCOADataset, KINSLVISDataset) on the hand-written annotation files under tests/golden/readers/.

Runs only in the build container (needs /root/reference; never on the GPU box).  The reference is imported unmodified
under the shims of make_golden.py; what its readers take from modules that are absent here is bound as follows:
``np.int`` = int; ``cvb.load`` = json.load of the named file; ``COCO`` = a minimal stand-in with ``loadImgs`` /
``loadAnns``; ``maskUtils.frPyObjects`` / ``merge`` / ``decode`` = this package's ``PolyMasks.from_coco(...).to_dense()``
(as ``cv2.resize`` is bound to the oracle's restatement in make_golden.py).  The masks themselves are therefore NOT golden
values -- tests/test_poly_cpu.py and tests/test_rle_cpu.py hold the rasterisation to fixed vectors -- and are not stored;
stored is everything the reference's reader LOGIC decides: lengths, index lists, orders, categories, boxes (those of the
reference's own ``utils.mask_to_bbox`` included), file names and ids.

usage:  python tests/golden/make_golden_readers.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402

from instaorder_amd.poly import PolyMasks  # noqa: E402

FIX = os.path.join(HERE, "readers")


class _Obj(object):
    """what the stand-in ``frPyObjects`` / ``merge`` hand to ``decode``: a dense [h, w] mask"""

    def __init__(self, dense):
        self.dense = dense


class MaskUtils(object):
    @staticmethod
    def _one(seg, h, w):
        return PolyMasks.from_coco([seg], h, w).to_dense()[0]

    @staticmethod
    def frPyObjects(segm, h, w):
        if isinstance(segm, dict):                                   # an uncompressed run-length code -> one object
            return _Obj(MaskUtils._one(segm, h, w))
        return [_Obj(MaskUtils._one([p], h, w)) for p in segm]       # polygons -> one object each

    @staticmethod
    def merge(objs):
        out = np.zeros_like(objs[0].dense)
        for o in objs:
            out |= o.dense
        return _Obj(out)

    @staticmethod
    def decode(obj):
        def dense(o):
            if isinstance(o, _Obj):
                return o.dense
            h, w = o["size"]                                         # a run-length dict of the annotation file
            return MaskUtils._one(o, h, w)
        if isinstance(obj, list):
            return np.stack([dense(o) for o in obj], axis=-1)        # [h, w, k], as pycocotools
        return dense(obj)


class COCO(object):
    def __init__(self, fn):
        with open(fn) as f:
            data = json.load(f)
        self.imgs = dict((im["id"], im) for im in data["images"])
        self.anns = dict((a["id"], a) for a in data["annotations"])

    def loadImgs(self, ids):
        return [self.imgs[i] for i in (ids if isinstance(ids, (list, tuple)) else [ids])]

    def loadAnns(self, ids):
        return [self.anns[i] for i in (ids if isinstance(ids, (list, tuple)) else [ids])]


def load_reference_reader():
    mg.install_shims()
    from datasets import reader
    import utils

    def load(fn):
        with open(fn) as f:
            return json.load(f)

    reader.cvb.load = load
    reader.COCO = COCO
    reader.maskUtils = MaskUtils
    return reader, utils


def strs(xs):
    return np.array([str(x) for x in xs])


def image_rows(out, tag, rd, n, **kw):
    """categories, boxes, file names (and ids) of every image, flattened with per-image offsets"""
    cats, boxes, fns, ids, offs = [], [], [], [], [0]
    for i in range(n):
        r = rd.get_image_instances(i, **kw)
        cats += [int(c) for c in r[1]]
        boxes += [[float(v) for v in b] for b in r[2]]
        fns.append(r[4])
        if kw.get("with_id"):
            ids.append(int(r[5]))
        offs.append(len(cats))
    out[tag + "/category"] = np.array(cats, np.int64)
    out[tag + "/bboxes"] = np.array(boxes, np.float64).reshape(-1, 4)
    out[tag + "/offsets"] = np.array(offs, np.int64)
    out[tag + "/image_fn"] = strs(fns)
    if ids:
        out[tag + "/image_id"] = np.array(ids, np.int64)


def main():
    reader, utils = load_reference_reader()
    out = {}

    # ---- InstaOrder ----
    rd = reader.InstaOrderDataset(os.path.join(FIX, "instaorder_val2017.json"))
    n = rd.get_image_length()
    out["io/lengths"] = np.array([n, rd.get_instance_length(), rd.get_occlusion_length(), rd.get_geometric_length()], np.int64)
    out["io/indexing"] = np.array(rd.indexing, np.int64)
    out["io/occ_all"] = np.array(rd.occ_all_img_and_idx, np.int64)
    out["io/depth_img"] = np.array([rd.get_imgId_and_depth(k)[0] for k in range(len(rd.depth_all_img_and_order))], np.int64)
    out["io/depth_order"] = strs(rd.get_imgId_and_depth(k)[1] for k in range(len(rd.depth_all_img_and_order)))
    for i in range(n):
        out["io/occ/%d" % i] = np.asarray(rd.get_gt_ordering(i, "occlusion", rm_bidirec=0))
        for ro in (0, 1):
            out["io/depth/%d/rm_overlap%d" % (i, ro)] = np.stack(rd.get_gt_ordering(i, "depth", rm_overlap=ro))
    image_rows(out, "io", rd, n, with_id=True, with_gt=True)
    inst = [rd.get_instance(k) for k in range(rd.get_instance_length())]
    out["io/instance_bbox"] = np.array([r[1] for r in inst], np.float64)
    out["io/instance_category"] = np.array([r[2] for r in inst], np.int64)
    out["io/instance_fn"] = strs(r[3] for r in inst)

    # ---- COCOA ----
    rd = reader.COCOADataset(os.path.join(FIX, "cocoa.json"))
    n = rd.get_image_length()
    out["cocoa/lengths"] = np.array([n, rd.get_instance_length()], np.int64)
    out["cocoa/indexing"] = np.array(rd.indexing, np.int64)
    for i in range(n):
        out["cocoa/order/%d" % i] = np.asarray(rd.get_gt_ordering(i))
    image_rows(out, "cocoa", rd, n, with_id=True, with_gt=True)                         # boxes: utils.mask_to_bbox
    image_rows(out, "cocoa_nostuff", rd, n, with_id=True, with_gt=True, ignore_stuff=True)
    inst = [rd.get_instance(k, with_gt=True) for k in range(rd.get_instance_length())]
    out["cocoa/instance_bbox"] = np.array([r[1] for r in inst], np.float64)
    # the reference's own mask_to_bbox on small arrays: the rule the kernel and the NumPy path restate
    probe = np.zeros((4, 6, 9), np.uint8)
    probe[1, 2, 3] = 1
    probe[2, 1:5, 2:8] = 1
    probe[2, 0, 0] = 2                                                                  # not equal to 1: does not count
    probe[3] = 255
    out["rule/probe"] = probe
    out["rule/bbox"] = np.array([utils.mask_to_bbox(m) for m in probe], np.int64)

    # ---- KINS / LVIS ----
    for name in ("KINS", "LVIS"):
        rd = reader.KINSLVISDataset(name, os.path.join(FIX, name.lower() + ".json"))
        n = rd.get_image_length()
        tag = name.lower()
        out[tag + "/lengths"] = np.array([n, rd.get_instance_length()], np.int64)
        out[tag + "/img_ids"] = np.array(rd.img_ids, np.int64)
        image_rows(out, tag, rd, n, with_gt=False)
        inst = [rd.get_instance(k) for k in range(rd.get_instance_length())]
        out[tag + "/instance_bbox"] = np.array([r[1] for r in inst], np.float64)
        out[tag + "/instance_category"] = np.array([r[2] for r in inst], np.int64)
        out[tag + "/instance_fn"] = strs(r[3] for r in inst)
    try:
        reader.KINSLVISDataset("ADE", os.path.join(FIX, "kins.json")).get_image_instances(0)
    except Exception as e:    # noqa: BLE001
        out["kinslvis/no_such_dataset"] = strs([str(e)])

    path = os.path.join(HERE, "readers.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
