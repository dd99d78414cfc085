"""The annotation readers on the MI355X: ``io_mask_bbox_u8`` (csrc/mask_bbox.hip) against the NumPy rule on every shape at
which the kernel takes another path (one pixel, 63 / 64 / 65 columns, several 64-pixel chunks, more rows than one band, an
odd base address), COCOA's device boxes against the dense mode and the reference's, every reader's encoded masks decoded on
the device against its dense mode byte for byte, and the consumers -- two dataset classes and ``evaluate.evaluate`` -- over
both mask modes."""
import numpy as np
import pytest
import torch

import readers_cases as rc
from instaorder_amd import _lib, datasets, evaluate, readers
from instaorder_amd.poly import PolyMasks

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 63), (3, 5, 64), (4, 7, 65), (5, 37, 130), (2, 300, 33)]
PATTERNS = ("empty", "full", "corner", "foreign", "random")


def pattern(kind, n, H, W, seed):
    rs = np.random.RandomState(seed)
    m = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        if kind == "full":
            m[i] = 1
        elif kind == "corner":                                   # a single pixel, at each corner in turn
            y, x = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)][(seed + i) % 4]
            m[i, y, x] = 1
        elif kind == "foreign":                                  # values 2 and 255 everywhere but a few pixels equal to 1
            m[i] = rs.choice(np.array([0, 2, 255], np.uint8), size=(H, W))
            for _ in range(i):                                   # mask 0 has none: empty under == 1, not under != 0
                m[i, rs.randint(H), rs.randint(W)] = 1
        elif kind == "random":
            y0, x0 = rs.randint(H), rs.randint(W)
            y1, x1 = rs.randint(y0, H) + 1, rs.randint(x0, W) + 1
            m[i, y0:y1, x0:x1] = rs.rand(y1 - y0, x1 - x0) < 0.3
    return m


def on_device(m, odd):
    """the masks as a contiguous device tensor whose first byte lies at an odd address when ``odd``"""
    buf = torch.zeros(m.size + 64, dtype=torch.uint8, device="cuda")
    skip = (1 if odd else 0) + (-buf.data_ptr()) % 2
    t = buf[skip:skip + m.size].view(m.shape)
    t.copy_(torch.from_numpy(m))
    assert t.is_contiguous() and t.data_ptr() % 2 == (1 if odd else 0)
    return t


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_mask_bboxes_against_the_numpy_rule(shape):
    n, H, W = shape
    assert 300 > 4 * _lib.lib().io_mask_bbox_band_rows()                     # (2, 300, 33) has more rows than one band
    for k, kind in enumerate(PATTERNS):
        m = pattern(kind, n, H, W, 10 * k + n)
        t = on_device(m, odd=k % 2 == 0)
        for eq1 in (True, False):
            got = readers.mask_bboxes(t, predicate_eq1=eq1)
            want = readers.mask_bboxes_host(m, predicate_eq1=eq1)
            print(kind, shape, eq1, got.tolist())
            assert got.dtype == np.int32 and got.shape == (n, 5)
            assert np.array_equal(got, want), (kind, eq1)
        if kind == "empty":
            assert not readers.mask_bboxes(t).any()                          # [0, 0, 0, 0, 0] by mask_to_bbox's rule
        if kind == "foreign":
            assert readers.mask_bboxes(t)[0].tolist() == [0, 0, 0, 0, 0]     # 2 and 255 do not count
        if kind == "corner":
            assert (readers.mask_bboxes(t)[:, 2:] == 1).all()


def test_no_masks_no_launch():
    t = torch.zeros((0, 5, 7), dtype=torch.uint8, device="cuda")
    got = readers.mask_bboxes(t)
    assert got.shape == (0, 5) and got.dtype == np.int32
    out = torch.full((5,), 77, dtype=torch.int32, device="cuda")
    rc_ = _lib.lib().io_mask_bbox_u8(t.data_ptr(), 0, 5, 7, 1, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc_ == 0 and (out.cpu() == 77).all()


def test_bboxes_do_not_depend_on_the_stream_or_repeat():
    """the accumulator is initialised by the call itself: a second call on the same output gives the same integers"""
    m = pattern("random", 5, 37, 130, 3)
    t = on_device(m, odd=True)
    first = readers.mask_bboxes(t)
    with torch.cuda.stream(torch.cuda.Stream()):
        again = readers.mask_bboxes(t)
    assert np.array_equal(first, again) and np.array_equal(first, readers.mask_bboxes_host(m))


def test_cocoa_encoded_boxes_equal_dense_and_the_reference():
    g = rc.golden()
    enc, den = rc.cocoa("encoded"), rc.cocoa("dense")
    for tag, stuff in (("cocoa", False), ("cocoa_nostuff", True)):
        offs = g[tag + "/offsets"]
        for i in range(enc.get_image_length()):
            a = enc.get_image_instances(i, with_gt=True, ignore_stuff=stuff)
            b = den.get_image_instances(i, with_gt=True, ignore_stuff=stuff)
            assert isinstance(a[0], PolyMasks) and isinstance(a[3], PolyMasks)
            assert np.array_equal(a[2], b[2]) and a[2].dtype == b[2].dtype
            assert np.array_equal(np.asarray(a[2], np.float64).reshape(-1, 4), g[tag + "/bboxes"][offs[i]:offs[i + 1]])
            assert np.array_equal(a[1], b[1]) and a[4] == b[4]
            assert enc.get_image_instances(i, ignore_stuff=stuff)[0] is a[0]              # cached with its boxes
    modal, _, bboxes, amodal = enc.get_image_instances(0, with_gt=True)[:4]
    assert not modal.to_dense()[2].any()                                                 # the fully hidden region ...
    assert list(bboxes[2]) == readers.mask_to_bbox(amodal.to_dense()[2]) and bboxes[2][2] > 0    # ... takes its amodal box
    for k in range(enc.get_instance_length()):
        assert np.array_equal(np.asarray(enc.get_instance(k)[1], np.float64), g["cocoa/instance_bbox"][k])


def _all_images(make):
    enc, den = make("encoded"), make("dense")
    for i in range(enc.get_image_length()):
        yield enc.get_image_instances(i, with_gt=True), den.get_image_instances(i, with_gt=True)


@pytest.mark.parametrize("which", ["InstaOrder", "COCOA", "KINS", "LVIS"])
def test_encoded_masks_decode_to_the_dense_mode_bytes(which):
    make = {"InstaOrder": rc.insta, "COCOA": rc.cocoa, "KINS": lambda m: rc.kinslvis("KINS", m),
            "LVIS": lambda m: rc.kinslvis("LVIS", m)}[which]
    seen = 0
    for a, b in _all_images(make):
        got = a[0].to_device("cuda").cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == b[0].shape and got.tobytes() == b[0].tobytes()
        if which != "InstaOrder":
            assert a[3].to_device("cuda").cpu().numpy().tobytes() == b[3].tobytes()
        seen += got.shape[0]
    assert seen >= 3


@pytest.mark.parametrize("cls,algo", [(datasets.SupOcclusionOrderBatches, "InstaOrderNet_o"),
                                      (datasets.SupDepthOccOrderBatches, "InstaOrderNet_od")])
def test_batches_are_bit_identical_over_both_mask_modes(cls, algo):
    load_image = rc.image_loader(rc.insta_image_sizes())
    out = {}
    for masks in rc.MODES:
        ds = cls(rc.data_cfg(64), "train", algo, rc.insta(masks), load_image, rng=np.random.RandomState(5))
        out[masks] = [t.cpu() for t in ds.batch([i % len(ds) for i in range(8)])]
        if masks == "encoded":
            assert ds.renderer.last_upload["masks"] < 8 * 2 * 33 * 65                    # vertices and runs, not pixels
    assert len(out["dense"]) == len(out["encoded"]) == (4 if algo == "InstaOrderNet_o" else 7)
    for a, b in zip(out["dense"], out["encoded"]):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert out["dense"][0].shape == (8, 3, 64, 64) and float(out["dense"][1].sum()) > 0


@pytest.mark.parametrize("kind", ["SupOcclusionOrderDataset", "SupDepthOrderDataset"])
def test_evaluate_device_rules_on_encoded_equals_host_on_dense(kind):
    cfg = rc.data_cfg(64, trainval_dataset=kind)
    load_image = rc.image_loader(rc.insta_image_sizes())
    dev = evaluate.evaluate(None, rc.insta("encoded"), load_image, cfg, "area", mask_rules="device", return_orders=True)
    hst = evaluate.evaluate(None, rc.insta("dense"), load_image, cfg, "area", mask_rules="host", return_orders=True)
    assert dev["num_test_images"] == hst["num_test_images"] == 3
    for k in hst:
        if k != "orders":
            assert dev[k] == hst[k], k
    for i in hst["orders"]:
        for a, b in zip(dev["orders"][i], hst["orders"][i]):
            assert (a is None and b is None) or np.array_equal(a, b)
