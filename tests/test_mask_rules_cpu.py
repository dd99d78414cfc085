"""CPU tests of the device mask rules (instaorder_amd.mask_rules): the C ABI exports them, bad input is refused before any
launch, and without a gfx950 device the 'device' path fails loudly.  No kernel is launched here."""
import numpy as np
import pytest
import torch

from helpers import synthetic
from instaorder_amd import _lib, evaluate, inference, mask_rules

NEW_SYMBOLS = ("io_mask_pack", "io_mask_pair_counts", "io_instance_depth_select", "io_instance_depth_select_workspace_bytes")


def test_new_symbols_are_exported_with_signatures():
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["io_mask_pack"][1]) == 9
    assert len(_lib.SIGNATURES["io_mask_pair_counts"][1]) == 8
    assert len(_lib.SIGNATURES["io_instance_depth_select"][1]) == 13


def test_workspace_bytes_grow_with_n_and_refuse_bad_shapes():
    lib = _lib.lib()
    assert lib.io_instance_depth_select_workspace_bytes(0, 10, 10) == 0
    assert lib.io_instance_depth_select_workspace_bytes(3, 0, 10) == 0
    assert lib.io_instance_depth_select_workspace_bytes(3, 10, -1) == 0
    a = lib.io_instance_depth_select_workspace_bytes(1, 480, 640)
    b = lib.io_instance_depth_select_workspace_bytes(40, 480, 640)
    assert 0 < a < b


def _masks():
    m = np.zeros((3, 8, 9), np.uint8)
    m[0, 1:3, 1:3] = 1
    m[1, 3:5, 1:3] = 1
    m[2, 6:8, 6:8] = 1
    return m


@pytest.mark.parametrize("bad", [
    np.zeros((8, 9), np.uint8),                                   # ndim
    np.zeros((1, 2, 8, 9), np.uint8),                             # ndim
    np.zeros((2, 8, 9), np.complex64),                            # dtype
    np.array([[["a"]]]),                                          # dtype
    np.full((2, 8, 9), 256, np.int32),                            # value > 255
    np.full((2, 8, 9), -1, np.int64),                             # value < 0
    np.full((2, 8, 9), 0.5, np.float32),                          # not an integer
    np.zeros((2, 0, 9), np.uint8),                                # empty image
    torch.zeros(8, 9, dtype=torch.uint8),                         # ndim (tensor)
    torch.zeros(2, 8, 9, dtype=torch.complex64),                  # dtype (tensor)
    torch.full((2, 8, 9), 300.0),                                 # value > 255 (tensor)
])
def test_bad_masks_raise_value_error(bad):
    for fn in (lambda m: mask_rules.pair_relations(m), lambda m: mask_rules.select_pairs(m, "nbor"),
               lambda m: mask_rules.infer_occ_order_area(m), lambda m: mask_rules.infer_depth_order_yaxis(m),
               lambda m: mask_rules.infer_gt_order(m, m),
               lambda m: mask_rules.depth_orders_from_disp(torch.zeros(8, 9), m, [], "median")):
        with pytest.raises(ValueError):
            fn(bad)


def test_bad_pairs_and_amodal_shape_raise_value_error():
    m = _masks()
    with pytest.raises(ValueError):
        mask_rules.select_pairs(m, "some")
    with pytest.raises(ValueError):
        mask_rules.infer_gt_order(m, m[:2])
    with pytest.raises(ValueError):
        mask_rules.depth_orders_from_disp(torch.zeros(8, 9), m, [(0, 3)], "mean")
    with pytest.raises(ValueError):
        mask_rules.depth_orders_from_disp(torch.zeros(9, 9), m, [(0, 1)], "mean")


def test_bad_mask_rules_value_raises_value_error():
    m = _masks()
    rd = synthetic.SyntheticReader(3, n_images=1, n_inst=3, empty_every=0)
    cfg = dict(trainval_dataset="SupOcclusionOrderDataset", patch_or_image="patch", input_size=64, dataset="COCOA",
               enlarge_box=3.0)
    for bad in ("gpu", "", None, "DEVICE"):
        with pytest.raises(ValueError, match="mask_rules"):
            evaluate.evaluate(None, rd, rd.load_image, cfg, "area", mask_rules=bad)
        with pytest.raises(ValueError, match="mask_rules"):
            inference.infer_order_sup_depth(None, None, m, None, "all", "midas_pretrained", "resize", 64, "median",
                                            mask_rules=bad)
        with pytest.raises(ValueError, match="mask_rules"):
            inference.infer_order_sup_occ(None, None, m, None, "all", "InstaOrderNet_o", "patch", 64, mask_rules=bad)
        with pytest.raises(ValueError, match="mask_rules"):
            inference.infer_order_sup_occ_depth(None, None, m, None, "all", "InstaOrderNet_od", "patch", 64,
                                                mask_rules=bad)


def test_empty_instance_list_needs_no_device():
    z = np.zeros((0, 5, 7), np.uint8)
    assert mask_rules.select_pairs(z, "nbor") == []
    assert mask_rules.infer_gt_order(z, z).shape == (0, 0)
    assert mask_rules.infer_depth_order_area(z).shape == (0, 0)


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = _masks()
    for fn in (lambda: mask_rules.pair_relations(m), lambda: mask_rules.select_pairs(m, "nbor"),
               lambda: mask_rules.infer_occ_order_yaxis(m), lambda: mask_rules.infer_gt_order(m, m),
               lambda: mask_rules.depth_orders_from_disp(torch.rand(8, 9), m, [(0, 1)], "median")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    rd = synthetic.SyntheticReader(3, n_images=1, n_inst=3, empty_every=0)
    cfg = dict(trainval_dataset="SupDepthOrderDataset", patch_or_image="resize", input_size=64, dataset="InstaOrder",
               enlarge_box=3.0, remove_depth_overlap=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.evaluate(None, rd, rd.load_image, cfg, "area", mask_rules="device")
