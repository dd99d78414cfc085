"""What tests/test_readers_cpu.py and tests/test_gpu_readers.py share: the annotation fixtures under tests/golden/readers/,
the golden values of the reference's readers on them (tests/golden/readers.npz, made by tests/golden/make_golden_readers.py),
independent constructions of the expected masks, a seeded image loader and the dataset configuration."""
import json
import os
import zlib

import numpy as np

from helpers import GOLDEN, load_golden
from instaorder_amd import readers
from instaorder_amd.poly import PolyMasks

FIX = os.path.join(GOLDEN, "readers")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MODES = ("dense", "encoded")

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = load_golden("readers")
    return _golden


def fix(name):
    return os.path.join(FIX, name)


def load(name):
    with open(fix(name)) as f:
        return json.load(f)


def insta(masks, **kw):
    return readers.InstaOrderReader(fix("instaorder_val2017.json"), masks=masks, **kw)


def cocoa(masks, **kw):
    return readers.COCOAReader(fix("cocoa.json"), masks=masks, **kw)


def kinslvis(name, masks, **kw):
    return readers.KINSLVISReader(name, fix(name.lower() + ".json"), masks=masks, **kw)


def host(m):
    """a reader's masks as a uint8 [n, H, W] host array, whichever mode handed them out"""
    return m.to_dense() if isinstance(m, PolyMasks) else np.asarray(m)


# ---- the expected masks, built here from the json files without the readers -----------------------------------------
def insta_expected_masks():
    order, coco = load("instaorder_val2017.json"), load("instances_val2017.json")
    imgs = dict((im["id"], im) for im in coco["images"])
    anns = dict((a["id"], a) for a in coco["annotations"])
    out = []
    for a in order["annotations"]:
        im = imgs[a["image_id"]]
        out.append(PolyMasks.from_coco([anns[i]["segmentation"] for i in a["instance_ids"]], im["height"], im["width"]).to_dense())
    return out


def cocoa_expected_masks(ignore_stuff=False):
    """[(modal, amodal)] per image"""
    data = load("cocoa.json")
    out = []
    for im, a in zip(data["images"], data["annotations"]):
        regs = [r for r in a["regions"] if not (ignore_stuff and r["isStuff"])]
        H, W = im["height"], im["width"]
        out.append((PolyMasks.from_coco([r.get("visible_mask", [r["segmentation"]]) for r in regs], H, W).to_dense(),
                    PolyMasks.from_coco([[r["segmentation"]] for r in regs], H, W).to_dense()))
    return out


def kinslvis_expected_masks(name):
    """[(modal, amodal)] per image, images in first-seen order of the annotations"""
    data = load(name.lower() + ".json")
    size = dict((im["id"], (im["height"], im["width"])) for im in data["images"])
    ids = []
    for a in data["annotations"]:
        if a["image_id"] not in ids:
            ids.append(a["image_id"])
    out = []
    for i in ids:
        anns = [a for a in data["annotations"] if a["image_id"] == i]
        H, W = size[i]
        out.append((PolyMasks.from_coco([a["inmodal_seg" if name == "KINS" else "segmentation"] for a in anns], H, W).to_dense(),
                    PolyMasks.from_coco([a["segmentation"] for a in anns], H, W).to_dense()))
    return out


# ---- consumers ------------------------------------------------------------------------------------------------------
def image_loader(reader_images):
    """load_image(file name) -> uint8 [H, W, 3], seeded by the name; ``reader_images``: {file name: (H, W)}"""
    def load_image(fn):
        H, W = reader_images[fn]
        return np.random.RandomState(zlib.crc32(fn.encode()) & 0x7fffffff).randint(0, 256, (H, W, 3)).astype(np.uint8)
    return load_image


def insta_image_sizes():
    return dict((im["file_name"], (im["height"], im["width"])) for im in load("instances_val2017.json")["images"])


def data_cfg(size=64, **over):
    cfg = dict(input_size=size, patch_or_image="patch", data_mean=MEAN, data_std=STD, load_rgb=True, use_category=False,
               dataset="InstaOrder", remove_occ_bidirec=0, remove_depth_overlap=0, enlarge_box=3.0,
               base_aug=dict(flip=True, shift=[-0.2, 0.2], scale=[0.8, 1.2]))
    cfg.update(over)
    return cfg
