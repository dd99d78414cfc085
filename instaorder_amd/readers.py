"""Annotation readers: the reference's ``datasets/reader.py`` classes ``InstaOrderDataset``, ``COCOADataset`` and
``KINSLVISDataset`` with the standard library in place of ``pycocotools`` / ``cvbase`` / ``cv2``, and with the instance masks
kept ENCODED up to the device (DESIGN.md "Annotation readers").

The reference rasterises every instance of an image to a dense [n, H, W] array on the host on every
``get_image_instances`` call.  Here ``masks="encoded"`` (the default) hands out one ``poly.PolyMasks`` per image -- the
polygons' vertices and the run-length codes of the crowd regions as the annotation file holds them -- which the renderer
(``datasets.PairRenderer``), the mask rules and the inference drivers decode on the GPU.  The object is cached in a bounded
LRU, and the SAME object comes back for the same image, so a batch that references an image several times uploads it once
(``datasets._Batches._render`` deduplicates by ``id(modal)``).  ``masks="dense"`` sends the same objects through
``to_dense()`` and returns the uint8 [n, H, W] arrays the reference returns.

One quantity of the reference comes from pixels and cannot come from an encoded mask on the host: COCOA's boxes
(``utils.mask_to_bbox`` of the visible mask, or of the amodal one where no pixel is visible).  ``COCOAReader`` in encoded
mode decodes the visible masks of an image once on the device and reads the boxes there (``mask_bboxes``,
``io_mask_bbox_u8`` of csrc/mask_bbox.hip); the boxes are cached with the masks.

The method surface -- names, argument order, tuple arities -- is the reference's, so ``datasets._Batches``,
``evaluate.evaluate`` and a reference-shaped trainer or tester take these classes unchanged.  Malformed annotations raise
``ValueError`` naming the file, the image index and the field.
"""
import collections
import json
import os
import re
import threading

import numpy as np

from . import _lib
from .poly import PolyMasks

_MODES = ("encoded", "dense")
_LT = re.compile(r"^\s*(\d+)\s*<\s*(\d+)\s*$")
_EQ = re.compile(r"^\s*(\d+)\s*=\s*(\d+)\s*$")
_BI = re.compile(r"^\s*(\d+)\s*<\s*(\d+)\s*&\s*(\d+)\s*<\s*(\d+)\s*$")
_DASH = re.compile(r"^\s*(\d+)\s*-\s*(\d+)\s*$")


def _load_json(fn):
    with open(fn, "r") as f:
        return json.load(f)


def mask_to_bbox(mask):
    """utils/data_utils.py:75-84 in NumPy: [x, y, w, h] of the pixels equal to 1, [0, 0, 0, 0] when there is none."""
    m = np.asarray(mask) == 1
    if not m.any():
        return [0, 0, 0, 0]
    rows, cols = np.where(m.any(axis=1))[0], np.where(m.any(axis=0))[0]
    return [int(cols[0]), int(rows[0]), int(cols[-1]) + 1 - int(cols[0]), int(rows[-1]) + 1 - int(rows[0])]


def mask_bboxes_host(masks, predicate_eq1=True):
    """What ``mask_bboxes`` computes, in NumPy on a host array [n, H, W]: int32 [n, 5] = x, y, w, h, count."""
    m = np.asarray(masks)
    out = np.zeros((m.shape[0], 5), np.int32)
    for i in range(m.shape[0]):
        p = (m[i] == 1) if predicate_eq1 else (m[i] != 0)
        out[i, :4] = mask_to_bbox(p.astype(np.uint8))
        out[i, 4] = int(p.sum())
    return out


def mask_bboxes(masks_u8_device, predicate_eq1=True):
    """int32 [n, 5] = x, y, w, h, count of the pixels equal to 1 (``predicate_eq1``) or different from 0 of every mask of a
    contiguous uint8 DEVICE tensor [n, H, W]: ``io_mask_bbox_u8``, enqueued on the current stream, then one copy to the
    host.  A mask without such a pixel gives a row of zeros (``mask_to_bbox``'s rule)."""
    import torch
    t = masks_u8_device
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or not t.is_cuda or not t.is_contiguous():
        raise ValueError("mask_bboxes: a contiguous uint8 device tensor [n, H, W] is expected")
    n, H, W = (int(v) for v in t.shape)
    if n == 0:
        return np.zeros((0, 5), np.int32)
    _lib.require_gpu()
    out = torch.empty((n, 5), dtype=torch.int32, device=t.device)
    rc = _lib.lib().io_mask_bbox_u8(t.data_ptr(), n, H, W, 1 if predicate_eq1 else 0, out.data_ptr(),
                                    torch.cuda.current_stream(t.device).cuda_stream)
    _lib.check(rc, "io_mask_bbox_u8")
    return out.cpu().numpy()


class _LRU(object):
    """the last ``size`` images' entries; ``get`` refreshes, ``put`` evicts the least recently used"""

    def __init__(self, size):
        if int(size) < 1:
            raise ValueError("cache_images must be at least 1 (got %r)" % (size,))
        self.size = int(size)
        self._d = collections.OrderedDict()
        self._lock = threading.Lock()

    def get(self, key):
        with self._lock:
            if key in self._d:
                self._d.move_to_end(key)
                return self._d[key]
        return None

    def put(self, key, value):
        with self._lock:
            self._d[key] = value
            self._d.move_to_end(key)
            while len(self._d) > self.size:
                self._d.popitem(last=False)
        return value

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d


class _Reader(object):
    def __init__(self, annot_fn, masks, cache_images):
        if masks not in _MODES:
            raise ValueError("masks must be 'encoded' or 'dense' (got %r)" % (masks,))
        self.annot_fn = annot_fn
        self.masks = masks
        self._cache = _LRU(cache_images)

    def _bad(self, imgidx, field, what, fn=None):
        return ValueError("%s: image %d: %s: %s" % (fn or self.annot_fn, imgidx, field, what))

    def _build(self, segs, H, W, imgidx, field):
        try:
            return PolyMasks.from_coco(segs, H, W)
        except ValueError as e:
            raise self._bad(imgidx, field, str(e))

    def _out(self, m):
        """a cached PolyMasks as the mask mode hands it out"""
        return m if self.masks == "encoded" else m.to_dense()

    def _one(self, m, i):
        """instance i for get_instance: the one-mask PolyMasks (shape (1, H, W)) or the dense [H, W] array"""
        return m[i] if self.masks == "encoded" else m[i].to_dense()[0]


# ---- InstaOrder (datasets/reader.py:294-457) ------------------------------------------------------------------------
class InstaOrderReader(_Reader):
    """``InstaOrderDataset``: the InstaOrder order file next to COCO's ``instances_{train2017|val2017}.json`` (derived from
    ``annot_fn`` as reader.py:299-306 does unless ``coco_annot_fn`` names it).  Images are indexed by id; of COCO's
    annotations only those whose id occurs in some ``instance_ids`` are kept.  Boxes and categories are the COCO
    annotation's; ``amodal`` is empty.

    ``get_gt_ordering`` returns the reference's matrices for ``rm_bidirec=0`` and ``rm_overlap`` 0 / 1.  With
    ``rm_bidirec=1`` the reference reads ``idx1, idx2`` before it assigns them (reader.py:346-348: the indices of the
    PREVIOUS entry, or a NameError on the first); no config sets it.  Implemented here is the evident intent: both
    directions of THAT bidirectional entry become -1."""

    def __init__(self, annot_fn, coco_annot_fn=None, masks="encoded", cache_images=256):
        super(InstaOrderReader, self).__init__(annot_fn, masks, cache_images)
        self.annot_info = _load_json(annot_fn)["annotations"]
        if coco_annot_fn is None:
            data_type = None
            for dtype in ("train2017", "val2017"):
                if dtype in annot_fn:
                    data_type = dtype
            if data_type is None:
                raise ValueError("%s: neither 'train2017' nor 'val2017' in the name: pass coco_annot_fn" % annot_fn)
            coco_annot_fn = os.path.join(os.path.dirname(annot_fn), "instances_%s.json" % data_type)
        self.coco_annot_fn = coco_annot_fn
        coco = _load_json(coco_annot_fn)
        wanted = set()
        for imgidx, ann in enumerate(self.annot_info):
            for a in ann["instance_ids"]:
                wanted.add(int(a))
        self._imgs = dict((im["id"], im) for im in coco["images"])
        self._anns = dict((a["id"], a) for a in coco["annotations"] if a["id"] in wanted)
        del coco
        for imgidx, ann in enumerate(self.annot_info):
            if ann["image_id"] not in self._imgs:
                raise self._bad(imgidx, "image_id", "image id %r is not in %s" % (ann["image_id"], coco_annot_fn))
            for a in ann["instance_ids"]:
                if int(a) not in self._anns:
                    raise self._bad(imgidx, "instance_ids", "COCO annotation id %r is not in %s" % (a, coco_annot_fn))

    # ---- lengths and index lists ----
    def get_image_length(self):
        return len(self.annot_info)

    def get_instance_length(self):
        self.indexing = [(i, k) for i, ann in enumerate(self.annot_info) for k in range(len(ann["instance_ids"]))]
        return len(self.indexing)

    def get_occlusion_length(self):
        self.occ_all_img_and_idx = [(i, k) for i, ann in enumerate(self.annot_info) for k in range(len(ann["occlusion"]))]
        return len(self.occ_all_img_and_idx)

    def get_geometric_length(self):
        self.depth_all_img_and_order = [(i, d["order"]) for i, ann in enumerate(self.annot_info) for d in ann["depth"]]
        return len(self.depth_all_img_and_order)

    def get_imgId_and_depth(self, depth_all_idx):
        if not hasattr(self, "depth_all_img_and_order"):
            self.get_geometric_length()
        return self.depth_all_img_and_order[depth_all_idx]

    # ---- orders ----
    def _pair(self, imgidx, field, text, num, forms):
        """the two instance indices of one order string; ``forms``: the regular expressions this field admits"""
        if isinstance(text, str):
            for rx in forms:
                m = rx.match(text)
                if m is None:
                    continue
                g = [int(v) for v in m.groups()]
                if rx is _BI and (g[2], g[3]) != (g[1], g[0]):
                    break
                if g[0] >= num or g[1] >= num:
                    raise self._bad(imgidx, field, "instance index out of range in %r (the image has %d instances)"
                                    % (text, num))
                return g[0], g[1]
        raise self._bad(imgidx, field, "order %r is neither 'a<b', 'a=b' nor 'a<b & b<a'" % (text,))

    def get_gt_ordering(self, imgidx, type, rm_bidirec=0, rm_overlap=0):
        ann = self.annot_info[imgidx]
        num = len(ann["instance_ids"])
        assert type in ["depth", "occlusion"], "order type should be ond of depth or occlusion"
        if type == "occlusion":
            gt_occ_matrix = np.zeros((num, num), dtype=int)
            for o in ann["occlusion"]:
                text = o["order"]
                idx1, idx2 = self._pair(imgidx, "occlusion", text, num, (_BI, _LT))
                if "&" in text and rm_bidirec == 1:
                    gt_occ_matrix[idx1, idx2] = -1
                    gt_occ_matrix[idx2, idx1] = -1
                elif "&" in text:
                    gt_occ_matrix[idx1, idx2] = 1
                    gt_occ_matrix[idx2, idx1] = 1
                else:
                    gt_occ_matrix[idx1, idx2] = 1
            return gt_occ_matrix
        gt_depth_matrix = np.ones((num, num), dtype=int) * (-1)
        is_overlap_matrix = np.ones((num, num), dtype=int) * (-1)
        count_matrix = np.ones((num, num), dtype=int) * (-1)
        for d in ann["depth"]:
            text, is_overlap, count = d["order"], d["overlap"], d["count"]
            idx1, idx2 = self._pair(imgidx, "depth", text, num, (_LT, _EQ))
            if rm_overlap and is_overlap:
                is_overlap_matrix[idx1, idx2] = is_overlap_matrix[idx2, idx1] = -1
            elif is_overlap:
                is_overlap_matrix[idx1, idx2] = is_overlap_matrix[idx2, idx1] = 1
            else:
                is_overlap_matrix[idx1, idx2] = is_overlap_matrix[idx2, idx1] = 0
            if "<" in text:
                gt_depth_matrix[idx1, idx2] = 1
                gt_depth_matrix[idx2, idx1] = 0
            else:
                gt_depth_matrix[idx1, idx2] = 2
                gt_depth_matrix[idx2, idx1] = 2
            count_matrix[idx1, idx2] = count_matrix[idx2, idx1] = count
        return [gt_depth_matrix, is_overlap_matrix, count_matrix]

    # ---- instances ----
    def _entry(self, idx):
        idx = int(idx)
        e = self._cache.get(idx)
        if e is None:
            ann_info = self.annot_info[idx]
            img_info = self._imgs[ann_info["image_id"]]
            anns = [self._anns[int(a)] for a in ann_info["instance_ids"]]
            modal = self._build(anns, img_info["height"], img_info["width"], idx, "segmentation")
            e = self._cache.put(idx, dict(modal=modal, anns=anns, image_fn=img_info["file_name"]))
        return e

    def get_instance(self, idx, with_gt=False):
        if not hasattr(self, "indexing"):
            self.get_instance_length()
        imgidx, regidx = self.indexing[idx]
        e = self._entry(imgidx)
        ann = e["anns"][regidx]
        return self._one(e["modal"], regidx), ann["bbox"], ann["category_id"], e["image_fn"], None

    def get_image_instances(self, idx, with_id=False, with_gt=False, with_anns=False, ignore_stuff=False):
        e = self._entry(idx)
        ann_info = self.annot_info[idx]
        ret = (self._out(e["modal"]), np.array([a["category_id"] for a in e["anns"]]),
               np.array([a["bbox"] for a in e["anns"]]), np.array([]), e["image_fn"])
        if with_anns:
            return ret + (ann_info, ann_info["image_id"])
        if with_id:
            return ret + (ann_info["image_id"],)
        return ret


# ---- COCOA (datasets/reader.py:49-66, 209-291) ----------------------------------------------------------------------
class COCOAReader(_Reader):
    """``COCOADataset``.  A region's modal mask is its ``visible_mask`` (a run-length code) when present, otherwise its
    single polygon ``segmentation``, which is also its amodal mask; the category is the constant 1; the box is
    ``mask_to_bbox`` of the modal mask, or of the amodal one when no pixel of the modal mask equals 1.  In encoded mode the
    boxes are read on ``device`` (``mask_bboxes``; the current device when None) the first time an image is asked for, and
    cached with its masks; in dense mode they are computed in NumPy."""

    def __init__(self, annot_fn, masks="encoded", device=None, cache_images=256):
        super(COCOAReader, self).__init__(annot_fn, masks, cache_images)
        data = _load_json(annot_fn)
        self.images_info = data["images"]
        self.annot_info = data["annotations"]
        self.device = device
        self.indexing = [(i, j) for i, ann in enumerate(self.annot_info) for j in range(len(ann["regions"]))]

    def get_instance_length(self):
        return len(self.indexing)

    def get_image_length(self):
        return len(self.images_info)

    def get_gt_ordering(self, imgidx):
        regions = self.annot_info[imgidx]["regions"]
        num = len(regions)
        gt_order_matrix = np.zeros((num, num), dtype=int)
        order_str = self.annot_info[imgidx]["depth_constraint"]
        if len(order_str) == 0:
            return gt_order_matrix
        for o in order_str.split(","):
            m = _DASH.match(o)
            if m is None:
                raise self._bad(imgidx, "depth_constraint", "entry %r is not 'a-b'" % (o,))
            idx1, idx2 = int(m.group(1)) - 1, int(m.group(2)) - 1
            if not (0 <= idx1 < num and 0 <= idx2 < num):
                raise self._bad(imgidx, "depth_constraint", "region index out of range in %r (the image has %d regions)"
                                % (o, num))
            if regions[idx2]["occlude_rate"] > 0.95:
                continue
            gt_order_matrix[idx1, idx2] = 1
        return gt_order_matrix

    def _boxes(self, modal, amodal):
        """int64 [n, 4]: mask_to_bbox(modal), mask_to_bbox(amodal) where the modal mask has no pixel equal to 1"""
        n = len(modal)
        if n == 0:
            return np.zeros((0, 4), np.int64)
        if self.masks == "dense":
            got = mask_bboxes_host(modal.to_dense())
            hidden = np.nonzero(got[:, 4] == 0)[0]
            if hidden.size:
                got[hidden] = mask_bboxes_host(amodal[hidden].to_dense())
            return got[:, :4].astype(np.int64)
        import torch
        _lib.require_gpu()
        device = torch.device("cuda", torch.cuda.current_device()) if self.device is None else torch.device(self.device)
        got = mask_bboxes(modal.to_device(device))                 # the decoded masks are scratch: only the boxes stay
        hidden = np.nonzero(got[:, 4] == 0)[0]
        if hidden.size:
            got[hidden] = mask_bboxes(amodal[hidden].to_device(device))
        return got[:, :4].astype(np.int64)

    def _entry(self, idx, ignore_stuff=False):
        key = (int(idx), bool(ignore_stuff))
        e = self._cache.get(key)
        if e is None:
            img_info = self.images_info[key[0]]
            H, W = img_info["height"], img_info["width"]
            regions = [r for r in self.annot_info[key[0]]["regions"] if not (ignore_stuff and r["isStuff"])]
            modal = self._build([r["visible_mask"] if "visible_mask" in r else [r["segmentation"]] for r in regions],
                                H, W, key[0], "regions")
            amodal = self._build([[r["segmentation"]] for r in regions], H, W, key[0], "regions")
            e = self._cache.put(key, dict(modal=modal, amodal=amodal, bboxes=self._boxes(modal, amodal),
                                          image_fn=img_info["file_name"]))
        return e

    def get_instance(self, idx, with_gt=False):
        imgidx, regidx = self.indexing[idx]
        e = self._entry(imgidx)
        return (self._one(e["modal"], regidx), [int(v) for v in e["bboxes"][regidx]], 1, e["image_fn"],
                self._one(e["amodal"], regidx) if with_gt else None)

    def get_image_instances(self, idx, with_id=False, with_gt=False, with_anns=False, ignore_stuff=False):
        e = self._entry(idx, ignore_stuff)
        n = len(e["modal"])
        ret = (self._out(e["modal"]), np.array([1] * n), e["bboxes"].copy() if n else np.array([]),
               self._out(e["amodal"]) if with_gt else np.array([]), e["image_fn"])
        if with_anns:
            return ret + (self.annot_info[idx], self.images_info[idx]["id"])
        if with_id:
            return ret + (self.images_info[idx]["id"],)
        return ret


# ---- KINS and LVIS (datasets/reader.py:20-46, 460-539) --------------------------------------------------------------
class KINSLVISReader(_Reader):
    """``KINSLVISDataset``.  'KINS': the modal mask is the run-length code ``inmodal_seg``, the box ``inmodal_bbox``;
    'LVIS': ``read_LVIS`` (``segmentation`` as polygons or a run-length code, the box ``bbox``).  Images are grouped by
    ``image_id`` in first-seen order.  With ``with_gt`` the amodal mask is the OR of the polygons in ``segmentation``."""

    def __init__(self, dataset, annot_fn, masks="encoded", cache_images=256):
        if dataset not in ("KINS", "LVIS"):
            raise Exception("No such dataset: {}".format(dataset))
        super(KINSLVISReader, self).__init__(annot_fn, masks, cache_images)
        self.dataset = dataset
        data = _load_json(annot_fn)
        self.images_info = data["images"]
        self.annot_info = data["annotations"]
        self.category_info = data["categories"]
        self.imgfn_dict = dict((a["id"], a["file_name"]) for a in self.images_info)
        self.size_dict = dict((a["id"], (a["width"], a["height"])) for a in self.images_info)
        self.anns_dict = self.make_dict()
        self.img_ids = list(self.anns_dict.keys())
        self._img_index = dict((imgid, k) for k, imgid in enumerate(self.img_ids))

    def make_dict(self):
        anns_dict = collections.OrderedDict()
        for ann in self.annot_info:
            anns_dict.setdefault(ann["image_id"], []).append(ann)
        return anns_dict

    def get_instance_length(self):
        return len(self.annot_info)

    def get_image_length(self):
        return len(self.img_ids)

    def _modal_field(self):
        return "inmodal_seg" if self.dataset == "KINS" else "segmentation"

    def _box(self, ann):
        return ann["inmodal_bbox"] if self.dataset == "KINS" else ann["bbox"]

    def _entry(self, idx):
        idx = int(idx)
        e = self._cache.get(idx)
        if e is None:
            imgid = self.img_ids[idx]
            W, H = self.size_dict[imgid]
            anns = self.anns_dict[imgid]
            modal = self._build([a[self._modal_field()] for a in anns], H, W, idx, self._modal_field())
            e = self._cache.put(idx, dict(modal=modal, amodal=None, anns=anns, H=H, W=W, image_fn=self.imgfn_dict[imgid]))
        return e

    def _amodal(self, e, idx):
        if e["amodal"] is None:
            e["amodal"] = self._build([a["segmentation"] for a in e["anns"]], e["H"], e["W"], idx, "segmentation")
        return e["amodal"]

    def get_instance(self, idx, with_gt=False):
        ann = self.annot_info[idx]
        imgidx = self._img_index[ann["image_id"]]
        e = self._entry(imgidx)
        k = next(k for k, a in enumerate(e["anns"]) if a is ann)
        return (self._one(e["modal"], k), self._box(ann), ann["category_id"], e["image_fn"],
                self._one(self._amodal(e, imgidx), k) if with_gt else None)

    def get_image_instances(self, idx, with_gt=False, with_anns=False):
        e = self._entry(idx)
        anns = e["anns"]
        ret = (self._out(e["modal"]), np.array([a["category_id"] for a in anns]), np.array([self._box(a) for a in anns]),
               self._out(self._amodal(e, idx)) if with_gt else np.array([]), e["image_fn"])
        if with_anns:
            return ret + (anns,)
        return ret


# the reference's names: a trainer or tester written against datasets/reader.py takes these unchanged
InstaOrderDataset = InstaOrderReader
COCOADataset = COCOAReader
KINSLVISDataset = KINSLVISReader
