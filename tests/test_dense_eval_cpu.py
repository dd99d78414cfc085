"""Dense-disparity evaluation (instaorder_amd.dense_eval) without a GPU: the KITTI / DIW readers' parsing and crop
arithmetic, and a NumPy restatement of the reference's metrics held to the golden of the real reference
(tests/golden/dense_eval.npz, written by make_golden_dense.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, synthetic

KITTI_SEED, KITTI_DISP_SEED, DIW_SEED, DIW_DISP_SEED = 11, 21, 12, 22


def golden():
    g = np.load(os.path.join(GOLDEN, "dense_eval.npz"), allow_pickle=False)
    assert [int(v) for v in g["meta"]] == [KITTI_SEED, KITTI_DISP_SEED, DIW_SEED, DIW_DISP_SEED]
    return g


def restate_errors(pred, gt_raw, gt_div=256.0, min_depth=1e-3, max_depth=80.0):
    """test_disp_KITTI.py 'median' + compute_errors for one image, elementwise in fp32 in the reference's order, sums in
    fp64 -> ([abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, silog, n_valid, ratio], (median gt, median depth))."""
    f32 = np.float32
    gt = gt_raw.astype(f32) / f32(gt_div)
    valid = (gt >= f32(min_depth)) & (gt <= f32(max_depth))
    n = int(valid.sum())
    if n == 0:
        return np.array([np.nan] * 8 + [0.0, np.nan]), (np.float32(np.nan), np.float32(np.nan))
    norm = (pred - pred.min()) / pred.max()
    depth = f32(1) / (norm + f32(1e-3))
    mg, md = np.median(gt[valid]), np.median(depth[valid])
    ratio = f32(mg / md)
    depth = depth * ratio
    depth[depth < f32(min_depth)] = f32(min_depth)
    depth[depth > f32(max_depth)] = f32(max_depth)
    g, p = gt[valid], depth[valid]
    thr = np.maximum(g / p, p / g)
    diff = g - p
    sq = diff * diff
    ld = np.log(p) - np.log(g)
    d = lambda a: a.astype(np.float64)  # noqa: E731
    s_ld = d(ld).sum()
    row = [d(np.abs(diff) / g).sum() / n, d(sq / g).sum() / n, np.sqrt(d(sq).sum() / n), np.sqrt(d(ld * ld).sum() / n),
           (thr < f32(1.25)).sum() / n, (thr < f32(1.25 ** 2)).sum() / n, (thr < f32(1.25 ** 3)).sum() / n,
           np.sqrt(d(ld * ld).sum() / n - (s_ld / n) ** 2), float(n), float(ratio)]
    return np.array(row, np.float64), (np.float32(mg), np.float32(md))


def restate_sample(disp, h, w, y, x):
    """F.interpolate(disp[None, None], size=(h, w), mode='bilinear', align_corners=False)[y, x] on the CPU."""
    up = F.interpolate(torch.from_numpy(disp)[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
    return float(up[y, x])


def mini_kitti(root):
    from instaorder_amd import dense_eval
    lst = synthetic.write_mini_kitti(str(root), KITTI_SEED)
    return dense_eval.KITTIEigenReader(lst, str(root))


def mini_diw(root):
    from instaorder_amd import dense_eval
    csv_path = synthetic.write_mini_diw(str(root), DIW_SEED)
    return dense_eval.DIWReader(csv_path, str(root))


def test_kitti_reader_parsing_and_crop(tmp_path):
    from PIL import Image
    from instaorder_amd import dense_eval
    rd = mini_kitti(tmp_path)
    assert len(rd) == len(synthetic.MINI_KITTI_SIZES) == 3
    assert [rd.has_gt(i) for i in range(3)] == [True, False, True]
    assert rd.image_paths[0].startswith(str(tmp_path) + "/rawdata/2011_09_26/")
    assert rd.depth_paths[1].endswith("/data_depth_annotated/None")
    for i, (H, W) in enumerate(synthetic.MINI_KITTI_SIZES):
        img, box, gt = rd.load(i)
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        x, y = int((W - 1216) / 2), H - 352
        assert box == (x, y, 1216, 352)
        if i == 1:
            assert gt is None
            continue
        full = np.array(Image.open(rd.depth_paths[i]))
        assert gt.dtype == np.uint16 and gt.shape == (352, 1216)
        np.testing.assert_array_equal(gt, full[y:y + 352, x:x + 1216])
        assert 0.03 < (gt > 0).mean() < 0.07                      # ~5 % dense
    assert dense_eval.kitti_crop_box(375, 1242) == (13, 23, 1216, 352)
    assert dense_eval.kitti_crop_box(376, 1241) == (12, 24, 1216, 352)      # int() truncates the half pixel
    with pytest.raises(ValueError):
        dense_eval.kitti_crop_box(350, 1242)
    limited = dense_eval.KITTIEigenReader(os.path.join(str(tmp_path), "eigen_test.txt"), str(tmp_path), test_num=2)
    assert len(limited) == 2


def test_diw_reader_points_are_zero_based(tmp_path):
    from instaorder_amd import dense_eval
    rd = mini_diw(tmp_path)
    rows = open(os.path.join(str(tmp_path), "DIW_test.csv")).read().split("\n")
    assert len(rd) == len(synthetic.MINI_DIW_SIZES) == 6
    for i, (h, w) in enumerate(synthetic.MINI_DIW_SIZES):
        f = rows[2 * i + 1].split(",")
        assert rd.points[i] == tuple(int(v) - 1 for v in f[:4])
        assert rd.ordinals[i] == f[4][0]
        assert rd.image_paths[i] == "%s/%s" % (tmp_path, rows[2 * i][1:])
        img, pts, o = rd.load(i)
        assert img.shape == (h, w, 3) and img.dtype == np.uint8         # the grayscale thumbnail comes back as RGB
        assert pts == rd.points[i] and o == rd.ordinals[i]
    assert rd.ordinals[-1] == "=" and rd.points[-1][:2] == rd.points[-1][2:]
    bad = os.path.join(str(tmp_path), "bad.csv")
    with open(bad, "w") as f:
        f.write("./DIW_test/%s\n999,1,1,1,<,1,1\n" % os.path.basename(rd.image_paths[0]))
    with pytest.raises(ValueError):
        dense_eval.DIWReader(bad, str(tmp_path)).load(0)


def test_restated_metrics_match_reference_golden(tmp_path):
    g = golden()
    rd = mini_kitti(tmp_path)
    disps = synthetic.dense_disparities(KITTI_DISP_SEED, 3, 352, 1216)
    rows = []
    for i in range(3):
        _, _, gt = rd.load(i)
        if gt is not None:
            rows.append(restate_errors(disps[i], gt)[0])
    rows = np.array(rows)
    assert int(g["kitti_missing"]) == 1 and int(g["kitti_n"]) == len(rows) == 2
    ref = g["kitti_rows"]
    tol = np.array([1e-5] * 7 + [1e-4])          # silog: the reference's fp32 mean(d^2) - mean(d)^2 cancels
    assert np.all(np.abs(rows[:, :8] - ref) <= tol * np.abs(ref)), (rows[:, :8], ref)
    np.testing.assert_array_equal(rows[:, 4:7], ref[:, 4:7])     # a1..a3: exact counts over the same n
    assert np.all(np.abs(rows[:, :8].mean(0) - g["kitti_means"]) <= tol * np.abs(g["kitti_means"]))


def test_restated_ordinals_match_reference_golden(tmp_path):
    g = golden()
    rd = mini_diw(tmp_path)
    disps = synthetic.dense_disparities(DIW_DISP_SEED, len(rd), 384, 384)
    dec = []
    for i in range(len(rd)):
        img, (ay, ax, by, bx), _ = rd.load(i)
        h, w = img.shape[:2]
        a, b = restate_sample(disps[i], h, w, ay, ax), restate_sample(disps[i], h, w, by, bx)
        dec.append("<" if a > b else (">" if a < b else "="))
    assert [ord(c) for c in dec] == [int(v) for v in g["diw_decisions"]]
    wrong = sum(d != o for d, o in zip(dec, rd.ordinals))
    assert wrong == int(g["diw_wrong"]) and len(rd) == int(g["diw_total"])
    assert wrong / len(rd) * 100 == float(g["diw_whdr"])


def test_median_restatement_edge_cases():
    rs = np.random.RandomState(3)
    pred = (rs.randint(0, 50, size=(37, 53)) / np.float32(7)).astype(np.float32) + np.float32(0.5)
    for nvalid in (0, 1, 2, 7):
        gt = np.zeros((37, 53), np.uint16)
        gt.reshape(-1)[rs.choice(37 * 53, nvalid, replace=False)] = rs.randint(1, 80 * 256, size=nvalid)
        row, (mg, md) = restate_errors(pred, gt)
        assert row[8] == nvalid
        if nvalid == 0:
            assert np.isnan(row[:8]).all() and np.isnan(row[9])
            continue
        g = gt.astype(np.float32) / np.float32(256)
        assert mg == np.median(g[g > 0]) and np.isfinite(row[:8]).all()
        if nvalid == 2:                                   # even count: the fp32 mean of the two middle values
            a, b = np.sort(g[g > 0])
            assert mg == np.float32((a + b) / np.float32(2))


def test_symbols_are_declared():
    from instaorder_amd import _lib
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "instaorder_hip.h")).read()
    for name in ("io_depth_errors_median_workspace_bytes", "io_depth_errors_median", "io_disp_sample_points"):
        assert name in _lib.SIGNATURES and name + "(" in hdr
