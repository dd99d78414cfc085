"""CPU tests of the annotation readers (instaorder_amd.readers): both mask modes of the three readers against what the
REFERENCE's readers return on the same hand-written files (tests/golden/readers.npz), the dense masks against
``PolyMasks.from_coco(...).to_dense()`` of the same annotations, the documented ``rm_bidirec=1`` matrix, the refusals, the
cache, the import hygiene, the C ABI of ``io_mask_bbox_u8`` and the dataset classes' plans over both modes.  No kernel is
launched here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import readers_cases as rc
from helpers import ROOT
from instaorder_amd import _lib, datasets, readers
from instaorder_amd.poly import PolyMasks


def _rows(g, tag, rd, n, **kw):
    offs = g[tag + "/offsets"]
    for i in range(n):
        r = rd.get_image_instances(i, **kw)
        a, b = int(offs[i]), int(offs[i + 1])
        assert len(r[0]) == b - a
        assert np.array_equal(np.asarray(r[1]).reshape(-1), g[tag + "/category"][a:b])
        assert np.array_equal(np.asarray(r[2], np.float64).reshape(-1, 4), g[tag + "/bboxes"][a:b])
        assert r[4] == str(g[tag + "/image_fn"][i])
        if kw.get("with_id"):
            assert r[5] == int(g[tag + "/image_id"][i])
        yield i, r


@pytest.mark.parametrize("masks", rc.MODES)
def test_instaorder_reader_equals_the_reference(masks):
    g, rd = rc.golden(), rc.insta(masks)
    assert rd.coco_annot_fn == rc.fix("instances_val2017.json")                      # derived as reader.py:299-306 does
    n = rd.get_image_length()
    assert [n, rd.get_instance_length(), rd.get_occlusion_length(), rd.get_geometric_length()] == list(g["io/lengths"])
    assert np.array_equal(np.array(rd.indexing), g["io/indexing"])
    assert np.array_equal(np.array(rd.occ_all_img_and_idx), g["io/occ_all"])
    for k in range(len(g["io/depth_img"])):
        assert rd.get_imgId_and_depth(k) == (int(g["io/depth_img"][k]), str(g["io/depth_order"][k]))
    for i in range(n):
        occ = rd.get_gt_ordering(i, "occlusion", rm_bidirec=0)
        assert occ.dtype == g["io/occ/%d" % i].dtype and np.array_equal(occ, g["io/occ/%d" % i])
        assert np.array_equal(rd.get_gt_ordering(i, type="occlusion"), occ)
        for ro in (0, 1):
            dep = rd.get_gt_ordering(i, "depth", rm_overlap=ro)
            assert isinstance(dep, list) and len(dep) == 3
            assert np.array_equal(np.stack(dep), g["io/depth/%d/rm_overlap%d" % (i, ro)])
    expected = rc.insta_expected_masks()
    for i, r in _rows(g, "io", rd, n, with_id=True, with_gt=True):
        assert len(r) == 6 and np.asarray(r[3]).size == 0                            # amodal is empty
        assert isinstance(r[0], PolyMasks) == (masks == "encoded")
        if masks == "dense":
            assert r[0].dtype == np.uint8
        assert np.array_equal(rc.host(r[0]), expected[i])
    assert len(rd.get_image_instances(0)) == 5 and len(rd.get_image_instances(0, with_anns=True)) == 7
    r = rd.get_image_instances(1, with_anns=True, with_id=True)
    assert len(r) == 7 and r[5] is rd.annot_info[1] and r[6] == 25
    for k in range(rd.get_instance_length()):
        modal, bbox, cat, fn, amodal = rd.get_instance(k)
        i, j = rd.indexing[k]
        assert amodal is None and cat == int(g["io/instance_category"][k]) and fn == str(g["io/instance_fn"][k])
        assert np.array_equal(np.asarray(bbox, np.float64), g["io/instance_bbox"][k])
        assert np.array_equal(rc.host(modal).reshape(expected[i][j].shape), expected[i][j])


def test_instaorder_reader_keeps_only_referenced_annotations():
    rd = rc.insta("encoded")
    assert sorted(rd._anns) == [101, 102, 103, 104, 201, 202, 203, 301, 302]          # 998 and 999 of the COCO file are dropped
    explicit = readers.InstaOrderReader(rc.fix("instaorder_val2017.json"), coco_annot_fn=rc.fix("instances_val2017.json"))
    assert explicit.get_image_length() == 3
    assert readers.InstaOrderDataset is readers.InstaOrderReader and readers.COCOADataset is readers.COCOAReader
    assert readers.KINSLVISDataset is readers.KINSLVISReader


def test_rm_bidirec_1_marks_both_directions_of_that_entry():
    """the documented divergence: the reference reads idx1, idx2 before it assigns them (reader.py:346-348)"""
    rd = rc.insta("dense")
    want = np.array([[0, 1, 0, 0], [0, 0, -1, 0], [0, -1, 0, 0], [1, 0, 0, 0]])       # "0<1", "1<2 & 2<1", "3<0"
    assert np.array_equal(rd.get_gt_ordering(0, "occlusion", rm_bidirec=1), want)
    assert np.array_equal(rd.get_gt_ordering(0, "occlusion", 1), want)                # positional, as evaluate.evaluate calls it
    assert np.array_equal(rd.get_gt_ordering(2, "occlusion", rm_bidirec=1), rc.golden()["io/occ/2"])


@pytest.mark.parametrize("masks", rc.MODES)
def test_cocoa_reader_equals_the_reference(masks):
    g, rd = rc.golden(), rc.cocoa(masks)
    n = rd.get_image_length()
    assert [n, rd.get_instance_length()] == list(g["cocoa/lengths"])
    assert np.array_equal(np.array(rd.indexing), g["cocoa/indexing"])
    for i in range(n):
        assert np.array_equal(rd.get_gt_ordering(i), g["cocoa/order/%d" % i])
    assert rd.get_gt_ordering(0)[0, 2] == 0 and rd.get_gt_ordering(0)[0, 1] == 1      # "1-3": region 3 is hidden (> 0.95)
    if masks == "encoded" and not torch.cuda.is_available():
        # the boxes of encoded masks are read on the device: without one the reader says so (tests/test_gpu_readers.py
        # holds the encoded boxes to the same golden values)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            rd.get_image_instances(0)
        return
    for tag, stuff in (("cocoa", False), ("cocoa_nostuff", True)):
        expected = rc.cocoa_expected_masks(stuff)
        for i, r in _rows(g, tag, rd, n, with_id=True, with_gt=True, ignore_stuff=stuff):
            assert len(r) == 6
            assert np.array_equal(rc.host(r[0]), expected[i][0]) and np.array_equal(rc.host(r[3]), expected[i][1])
    assert len(rd.get_image_instances(0, ignore_stuff=True)[0]) == 3
    assert np.asarray(rd.get_image_instances(0)[3]).size == 0                         # no amodal masks without with_gt
    assert len(rd.get_image_instances(0, with_anns=True)) == 7
    # the fully hidden region takes the box of its amodal polygon
    modal, category, bboxes = rd.get_image_instances(0)[:3]
    assert not rc.host(modal)[2].any() and list(bboxes[2]) == readers.mask_to_bbox(expected[0][1][2]) and bboxes[2][2] > 0
    for k in range(rd.get_instance_length()):
        m, bbox, cat, fn, amodal = rd.get_instance(k, with_gt=True)
        assert cat == 1 and np.array_equal(np.asarray(bbox, np.float64), g["cocoa/instance_bbox"][k])
        assert rd.get_instance(k)[4] is None


def test_mask_to_bbox_restates_the_reference_rule():
    g = rc.golden()
    assert np.array_equal(np.array([readers.mask_to_bbox(m) for m in g["rule/probe"]]), g["rule/bbox"])
    got = readers.mask_bboxes_host(g["rule/probe"])
    assert np.array_equal(got[:, :4], g["rule/bbox"]) and list(got[:, 4]) == [0, 1, 24, 0]
    assert list(readers.mask_bboxes_host(g["rule/probe"], predicate_eq1=False)[:, 4]) == [0, 1, 25, 54]


@pytest.mark.parametrize("masks", rc.MODES)
@pytest.mark.parametrize("name", ["KINS", "LVIS"])
def test_kinslvis_reader_equals_the_reference(name, masks):
    g, rd, tag = rc.golden(), rc.kinslvis(name, masks), name.lower()
    n = rd.get_image_length()
    assert [n, rd.get_instance_length()] == list(g[tag + "/lengths"])
    assert rd.img_ids == list(g[tag + "/img_ids"])                                    # first-seen order
    expected = rc.kinslvis_expected_masks(name)
    for i, r in _rows(g, tag, rd, n):
        assert len(r) == 5 and np.asarray(r[3]).size == 0
        assert np.array_equal(rc.host(r[0]), expected[i][0])
    for i in range(n):
        r = rd.get_image_instances(i, with_gt=True, with_anns=True)
        assert len(r) == 6 and r[5] is rd.anns_dict[rd.img_ids[i]]
        assert np.array_equal(rc.host(r[3]), expected[i][1])                          # OR of the polygons in segmentation
    for k in range(rd.get_instance_length()):
        m, bbox, cat, fn, amodal = rd.get_instance(k)
        assert amodal is None and cat == int(g[tag + "/instance_category"][k]) and fn == str(g[tag + "/instance_fn"][k])
        assert np.array_equal(np.asarray(bbox, np.float64), g[tag + "/instance_bbox"][k])


def test_no_such_dataset_raises_the_reference_text():
    with pytest.raises(Exception) as e:
        readers.KINSLVISReader("ADE", rc.fix("kins.json"))
    assert str(e.value) == str(rc.golden()["kinslvis/no_such_dataset"][0]) == "No such dataset: ADE"


def test_bad_arguments():
    with pytest.raises(ValueError, match="masks"):
        rc.insta("rle")
    with pytest.raises(ValueError, match="cache_images"):
        rc.insta("dense", cache_images=0)
    with pytest.raises(ValueError, match="train2017"):
        readers.InstaOrderReader(rc.fix("bad_index.json"))                            # no split in the name, no coco_annot_fn


def _message(fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    return str(e.value)


def test_malformed_annotations_name_file_image_and_field():
    coco = rc.fix("instances_val2017.json")
    msg = _message(readers.InstaOrderReader, rc.fix("bad_missing_ann.json"), coco_annot_fn=coco)
    assert "bad_missing_ann.json" in msg and "image 1" in msg and "instance_ids" in msg and "4242" in msg
    rd = readers.InstaOrderReader(rc.fix("bad_index.json"), coco_annot_fn=coco, masks="dense")
    assert rd.get_gt_ordering(0, "occlusion").sum() == 1                              # the well-formed image still reads
    msg = _message(rd.get_gt_ordering, 1, "occlusion")
    assert "bad_index.json" in msg and "image 1" in msg and "occlusion" in msg and "out of range" in msg
    msg = _message(rd.get_gt_ordering, 1, "depth")
    assert "bad_index.json" in msg and "image 1" in msg and "depth" in msg and "out of range" in msg
    rd = readers.InstaOrderReader(rc.fix("bad_order.json"), coco_annot_fn=coco)
    for i, kind, text in ((1, "occlusion", "0>1"), (1, "depth", "0<1 & 1<0"), (2, "occlusion", "0<1 & 0<1"), (2, "depth", "0-1")):
        msg = _message(rd.get_gt_ordering, i, kind)
        assert "bad_order.json" in msg and "image %d" % i in msg and kind in msg and repr(text) in msg


def test_malformed_cocoa_constraints(tmp_path):
    import json
    data = rc.load("cocoa.json")
    data["annotations"][0]["depth_constraint"] = "1-2,1-9"
    data["annotations"][1]["depth_constraint"] = "1<2"
    fn = str(tmp_path / "cocoa_bad.json")
    with open(fn, "w") as f:
        json.dump(data, f)
    rd = readers.COCOAReader(fn, masks="dense")
    msg = _message(rd.get_gt_ordering, 0)
    assert "cocoa_bad.json" in msg and "image 0" in msg and "depth_constraint" in msg and "out of range" in msg
    msg = _message(rd.get_gt_ordering, 1)
    assert "cocoa_bad.json" in msg and "image 1" in msg and "depth_constraint" in msg


def test_same_image_same_object_until_evicted():
    rd = rc.insta("encoded", cache_images=2)
    a = rd.get_image_instances(0)[0]
    assert rd.get_image_instances(0, with_gt=True)[0] is a and rd.get_image_instances(0, with_id=True)[0] is a
    b = rd.get_image_instances(1)[0]
    assert rd.get_image_instances(0)[0] is a and rd.get_image_instances(1)[0] is b    # two images fit
    rd.get_image_instances(2)                                                         # evicts the least recently used: 0
    assert len(rd._cache) == 2 and 0 not in rd._cache
    assert rd.get_image_instances(1)[0] is b
    a2 = rd.get_image_instances(0)[0]
    assert a2 is not a and np.array_equal(a2.to_dense(), a.to_dense())


def test_eviction_at_cache_images_1():
    rd = rc.kinslvis("KINS", "encoded", cache_images=1)
    a = rd.get_image_instances(0)[0]
    assert rd.get_image_instances(0)[0] is a
    b = rd.get_image_instances(1)[0]
    assert len(rd._cache) == 1 and rd.get_image_instances(1)[0] is b
    assert rd.get_image_instances(0)[0] is not a


def test_import_needs_no_third_party_reader_module():
    code = ("import sys; import instaorder_amd.readers as r; r.InstaOrderReader(%r, masks='dense').get_image_instances(0); "
            "bad = [m for m in ('pycocotools', 'cvbase', 'cv2') if m in sys.modules]; assert not bad, bad"
            % rc.fix("instaorder_val2017.json"))
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=120)
    import instaorder_amd
    assert instaorder_amd.readers is readers


def test_bbox_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    m = re.search(r"\bint io_mask_bbox_u8\(([^)]*)\);", header)
    assert m, "io_mask_bbox_u8 is not declared in include/instaorder_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params[-1].startswith("hipStream_t")                                       # the stream is the last argument
    res, args = _lib.SIGNATURES["io_mask_bbox_u8"]
    assert len(args) == len(params) == 7 and res is _lib._I
    lib = _lib.lib()
    assert hasattr(lib, "io_mask_bbox_u8") and hasattr(lib, "io_mask_bbox_band_rows")
    assert 0 < lib.io_mask_bbox_band_rows() < 300
    # refused before any launch; n == 0 is IO_OK without one (no device is touched)
    assert lib.io_mask_bbox_u8(None, 0, 4, 4, 1, None, None) == 0
    assert lib.io_mask_bbox_u8(None, -1, 4, 4, 1, None, None) == -1
    assert lib.io_mask_bbox_u8(None, 2, 4, 4, 1, None, None) == -1 and "null" in _lib.last_error()
    assert lib.io_mask_bbox_u8(None, 2, 0, 4, 1, None, None) == -1
    assert lib.io_mask_bbox_u8(None, 2, 4, 4, 7, None, None) == -1
    assert lib.io_mask_bbox_u8(None, 2, 1 << 16, 1 << 15, 1, None, None) == -1        # H * W >= 2^31
    with pytest.raises(ValueError):
        readers.mask_bboxes(np.zeros((1, 2, 2), np.uint8))                            # a host array
    with pytest.raises(ValueError):
        readers.mask_bboxes(torch.zeros(1, 2, 2, dtype=torch.uint8))                  # a host tensor


@pytest.mark.parametrize("cls,algo", [(datasets.SupOcclusionOrderBatches, "InstaOrderNet_o"),
                                      (datasets.SupDepthOccOrderBatches, "InstaOrderNet_od")])
def test_plans_do_not_depend_on_the_mask_mode(cls, algo):
    plans = {}
    for masks in rc.MODES:
        rd = rc.insta(masks)
        ds = cls(rc.data_cfg(), "train", algo, rd, None, rng=np.random.RandomState(11))
        plans[masks] = [ds.plan(i % len(ds)) for i in range(24)]
    keys = [k for k in plans["dense"][0] if k != "modal"]
    assert "box" in keys and "flip" in keys and "idx1" in keys
    boxes = set()
    for a, b in zip(plans["dense"], plans["encoded"]):
        for k in keys:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert isinstance(b["modal"], PolyMasks) and np.array_equal(a["modal"], b["modal"].to_dense())
        boxes.add(a["box"])
    assert len(boxes) > 12                                                            # the augmentation really drew
