"""Dense-disparity evaluation on the MI355X: io_depth_errors_median / io_disp_sample_points against the NumPy restatement
(test_dense_eval_cpu.py), the MiDaS disparity at rectangular and KITTI input shapes, the drivers of
instaorder_amd.dense_eval end to end against the reference golden, and tools/test_disp.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import GOLDEN, ROOT, rel_err, synthetic
from test_dense_eval_cpu import (DIW_DISP_SEED, KITTI_DISP_SEED, golden, mini_diw, mini_kitti, restate_errors,
                                 restate_sample)

pytestmark = pytest.mark.gpu


def _case_maps(H, W, seed):
    """8 images: valid counts 0, 1, 2 (even median), 3, ~5 %, 100 %, ~5 % with a heavily tied disparity, ~30 % beyond
    80 m; disparities uint16 / 1000 (ties everywhere) except image 6 (8 levels)."""
    rs = np.random.RandomState(seed)
    pred = synthetic.dense_disparities(seed + 1, 8, H, W)
    pred[6] = (rs.randint(0, 8, size=(H, W)) / np.float32(4)).astype(np.float32) + np.float32(0.25)
    gt = np.zeros((8, H, W), np.uint16)
    for b, n in ((1, 1), (2, 2), (3, 3)):
        gt[b].reshape(-1)[rs.choice(H * W, n, replace=False)] = rs.randint(1, 80 * 256, size=n)
    gt[4] = synthetic.sparse_gt_u16(rs, H, W)
    gt[5] = rs.randint(1, 80 * 256 + 1, size=(H, W)).astype(np.uint16)
    gt[6] = synthetic.sparse_gt_u16(rs, H, W)
    gt[7] = synthetic.sparse_gt_u16(rs, H, W, density=0.3, max_raw=65535)
    return pred, gt


def _run(pred, gt):
    from instaorder_amd import dense_eval
    p = torch.from_numpy(pred).cuda()
    g = torch.from_numpy(gt.view(np.int16)).cuda()
    med = torch.empty((pred.shape[0], 2), dtype=torch.float32, device="cuda")
    rows = dense_eval.depth_errors_median(p, g, medians=med)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), med.cpu().numpy()


@pytest.mark.parametrize("H,W", [(352, 1216), (37, 53)])
def test_depth_errors_match_restatement(H, W):
    pred, gt = _case_maps(H, W, 7 + H)
    rows, med = _run(pred, gt)
    for b in range(8):
        ref, (mg, md) = restate_errors(pred[b], gt[b])
        assert rows[b, 8] == ref[8], b
        if ref[8] == 0:
            assert np.isnan(rows[b, :8]).all() and np.isnan(rows[b, 9]) and np.isnan(med[b]).all()
            continue
        # both medians and the ratio bit-equal to np.median's
        assert med[b, 0].tobytes() == mg.tobytes() and med[b, 1].tobytes() == md.tobytes(), (b, med[b], mg, md)
        assert np.float32(rows[b, 9]).tobytes() == np.float32(ref[9]).tobytes()
        np.testing.assert_array_equal(rows[b, 4:7], ref[4:7])          # a1..a3: exact counts
        err = np.abs(rows[b, :8] - ref[:8])
        assert np.all(err <= 1e-6 * np.abs(ref[:8]) + 1e-12), (b, rows[b], ref)
    # bitwise the same row for any B and on a second run
    again, _ = _run(pred, gt)
    assert again.tobytes() == rows.tobytes()
    r3, _ = _run(pred[:3].copy(), gt[:3].copy())
    assert r3.tobytes() == rows[:3].tobytes()
    for b in (2, 5, 7):
        r1, _ = _run(pred[b:b + 1].copy(), gt[b:b + 1].copy())
        assert r1.tobytes() == rows[b:b + 1].tobytes(), b


def test_depth_errors_under_graph_capture():
    from instaorder_amd import dense_eval
    pred, gt = _case_maps(37, 53, 99)
    p = torch.from_numpy(pred).cuda()
    g = torch.from_numpy(gt.view(np.int16)).cuda()
    eager = dense_eval.depth_errors_median(p, g).cpu().numpy()
    out = torch.full((8, 10), -1.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dense_eval.depth_errors_median(p, g, out=out)         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dense_eval.depth_errors_median(p, g, out=out)
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == eager.tobytes()


def test_disp_sample_points_match_interpolate():
    from instaorder_amd import dense_eval
    rs = np.random.RandomState(5)
    cases = []
    for k in range(24):
        H, W = rs.randint(8, 200), rs.randint(8, 200)
        h, w = (rs.randint(H, 3 * H), rs.randint(W, 3 * W)) if k % 2 == 0 else (rs.randint(2, H + 1), rs.randint(2, W + 1))
        if k == 0:
            h, w = H, W                                    # same size: a copy
        cases.append((H, W, h, w))
    for H, W, h, w in cases:
        B = 5
        disp = (rs.randint(0, 65536, size=(B, H, W)) / np.float32(1000)).astype(np.float32)
        pts = np.stack([np.full(B, h), np.full(B, w), rs.randint(0, h, B), rs.randint(0, w, B), rs.randint(0, h, B),
                        rs.randint(0, w, B)], 1).astype(np.int32)
        pts[B - 1, 4:6] = pts[B - 1, 2:4]                  # A == B: '='
        vals, dec = dense_eval.disp_sample_points(torch.from_numpy(disp).cuda(), torch.from_numpy(pts))
        vals, dec = vals.cpu().numpy(), dec.cpu().numpy()
        for b in range(B):
            ra = restate_sample(disp[b], h, w, pts[b, 2], pts[b, 3])
            rb = restate_sample(disp[b], h, w, pts[b, 4], pts[b, 5])
            for got, ref in ((vals[b, 0], ra), (vals[b, 1], rb)):
                assert abs(float(got) - ref) <= 2 * np.spacing(np.float32(abs(ref))), (H, W, h, w, b, got, ref)
            want = "<" if ra > rb else (">" if ra < rb else "=")
            assert chr(dec[b]) == want, (H, W, h, w, b)


def _midas_state(net, seed):
    sd = net.state_dict()
    spec = [(k, tuple(v.shape), None) for k, v in sd.items()]
    vals = synthetic.make_spec_state_dict(seed, spec)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in vals.items()}, strict=True)
    return vals


@pytest.mark.parametrize("kind", ["MidasNet", "InstaDepthNet_d"])
def test_disparity_rectangular_matches_oracle(kind):
    """96 x 320 input: encoder stages 24x80 .. 3x10 (odd sizes), eval mode, against oracle.midas_oracle."""
    from instaorder_amd import midas_net
    from oracle import midas_oracle as mo
    net = getattr(midas_net, kind)(non_negative=True).cuda()
    vals = _midas_state(net, 31)
    net.eval()
    rs = np.random.RandomState(32)
    img = torch.from_numpy(rs.standard_normal((2, 3, 96, 320)).astype(np.float32))
    with torch.no_grad():
        got = (net(img.cuda()) if kind == "MidasNet" else net._encode_decode(img.cuda())[0]).cpu().numpy()
        st = mo.state_from_numpy(vals, prefix="")
        z = torch.zeros((2, 1, 96, 320))
        ref = mo.forward(st, img, z, z, False, "d" if kind == "InstaDepthNet_d" else "od")[0].numpy() \
            if kind == "InstaDepthNet_d" else _oracle_disp(mo, st, img)
    assert got.shape == (2, 96, 320)
    assert rel_err(got, ref) < 1e-3, rel_err(got, ref)


def _oracle_disp(mo, st, img):
    """the disparity part of midas_oracle.forward (MidasNet has no order branches)"""
    l1 = mo._layer1(st, "pretrained", img, 3, 32, False)
    l2 = mo._stage(st, "pretrained.layer2", l1, 4, 2, 32, False)
    l3 = mo._stage(st, "pretrained.layer3", l2, 23, 2, 32, False)
    l4 = mo._stage(st, "pretrained.layer4", l3, 3, 2, 32, False)
    rn = [F.conv2d(l, st["scratch.layer%d_rn.weight" % (i + 1)], padding=1) for i, l in enumerate((l1, l2, l3, l4))]
    p4 = mo._fusion(st, "scratch.refinenet4", rn[3])
    p3 = mo._fusion(st, "scratch.refinenet3", p4, rn[2])
    p2 = mo._fusion(st, "scratch.refinenet2", p3, rn[1])
    p1 = mo._fusion(st, "scratch.refinenet1", p2, rn[0])
    y = F.conv2d(p1, st["scratch.output_conv.0.weight"], st["scratch.output_conv.0.bias"], padding=1)
    y = F.interpolate(y, scale_factor=2, mode="bilinear", align_corners=False)
    y = F.relu(F.conv2d(y, st["scratch.output_conv.2.weight"], st["scratch.output_conv.2.bias"], padding=1))
    y = F.relu(F.conv2d(y, st["scratch.output_conv.4.weight"], st["scratch.output_conv.4.bias"]))
    return y[:, 0].numpy()


def test_kitti_shape_batch_equals_single_images():
    from instaorder_amd import midas_net
    net = midas_net.MidasNet(non_negative=True).cuda()
    _midas_state(net, 41)
    net.eval()
    rs = np.random.RandomState(42)
    img = torch.from_numpy(rs.standard_normal((4, 3, 352, 1216)).astype(np.float32)).cuda()
    with torch.no_grad():
        batched = net(img)
        singles = torch.cat([net(img[i:i + 1]) for i in range(4)], 0)
    torch.cuda.synchronize()
    assert batched.shape == (4, 352, 1216)
    assert torch.isfinite(batched).all()
    assert rel_err(batched.cpu().numpy(), singles.cpu().numpy()) < 1e-5


def test_kitti_render_equals_reference_normalisation(tmp_path):
    from instaorder_amd import dense_eval
    rd = mini_kitti(tmp_path)
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    ren = dense_eval._renderer((352, 1216), mean, std, torch.device("cuda", 0))
    imgs, boxes = [], []
    for i in range(3):
        img, box, _ = rd.load(i)
        imgs.append(img)
        boxes.append(box)
    rgb = dense_eval.render_rgb(ren, imgs, boxes).cpu()
    for i, (img, (x, y, w, h)) in enumerate(zip(imgs, boxes)):
        crop = torch.from_numpy(img[y:y + h, x:x + w].transpose(2, 0, 1).astype(np.float32))
        ref = (crop / 255. - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
        d = (rgb[i] - ref).abs()
        assert float((d / torch.finfo(torch.float32).eps / ref.abs().clamp_min(1e-30)).max()) <= 1.0, i


class _StubNet(object):
    """_encode_decode(rgb) -> the next golden disparity maps (in reader order of the evaluated images)"""

    def __init__(self, disps):
        self.disps, self.k = disps, 0

    def _encode_decode(self, rgb):
        B = rgb.shape[0]
        assert rgb.is_cuda and rgb.dtype == torch.float32
        d = torch.from_numpy(self.disps[self.k:self.k + B].copy()).to(rgb.device)
        self.k += B
        return d, None


def test_eval_dense_depth_matches_reference_golden(tmp_path):
    from instaorder_amd import dense_eval
    g = golden()
    rd = mini_kitti(tmp_path)
    disps = synthetic.dense_disparities(KITTI_DISP_SEED, 3, 352, 1216)
    present = [i for i in range(3) if rd.has_gt(i)]
    for batch in (1, 4):
        r = dense_eval.eval_dense_depth(_StubNet(disps[present]), rd, "midas_pretrained", batch=batch, return_rows=True)
        assert r["missing"] == int(g["kitti_missing"]) and r["n_images"] == int(g["kitti_n"])
        tol = np.array([1e-5] * 7 + [1e-4])
        means = np.array([r[k] for k in dense_eval.ERROR_NAMES])
        assert np.all(np.abs(means - g["kitti_means"]) <= tol * np.abs(g["kitti_means"])), (means, g["kitti_means"])
        np.testing.assert_array_equal(r["rows"][:, 4:7], g["kitti_rows"][:, 4:7])


def test_eval_ordinal_via_disp_matches_reference_golden(tmp_path):
    from instaorder_amd import dense_eval
    g = golden()
    rd = mini_diw(tmp_path)
    disps = synthetic.dense_disparities(DIW_DISP_SEED, len(rd), 384, 384)
    for batch in (8, 4):
        r = dense_eval.eval_ordinal_via_disp(_StubNet(disps), rd, "midas_pretrained", batch=batch, return_decisions=True)
        assert [ord(c) for c in r["decisions"]] == [int(v) for v in g["diw_decisions"]]
        assert r["wrong"] == int(g["diw_wrong"]) and r["total"] == int(g["diw_total"])
        assert r["WHDR"] == float(g["diw_whdr"])


@pytest.mark.parametrize("dataset,algo", [("kitti", "InstaDepthNet_d"), ("diw", "midas_pretrained")])
def test_tools_test_disp_runs(tmp_path, dataset, algo):
    import yaml
    from instaorder_amd import midas_net
    if dataset == "kitti":
        lst = synthetic.write_mini_kitti(str(tmp_path), 11)
        data = dict(dataset="kitti", val_image_root=str(tmp_path), val_annot_file=lst)
    else:
        csv_path = synthetic.write_mini_diw(str(tmp_path), 12)
        data = dict(dataset="diw", base_dir="", val_image_root=str(tmp_path), val_annot_file=csv_path)
    data.update(data_mean=[0.485, 0.456, 0.406], data_std=[0.229, 0.224, 0.225])
    model = dict(algo=algo, use_rgb=True, lr=1e-5, optim="SGD", weight_decay=1e-4, backbone_arch=algo,
                 backbone_param=dict(in_channels=5, num_classes=3), inmask_weight=5.0)
    net = (midas_net.InstaDepthNet_d if algo == "InstaDepthNet_d" else midas_net.MidasNet)(non_negative=True)
    _midas_state(net, 51)
    ck = os.path.join(str(tmp_path), "ckpt_iter_7.pth.tar")
    if algo == "midas_pretrained":
        torch.save(net.state_dict(), ck)
    else:
        torch.save({"step": 7, "state_dict": {"module." + k: v for k, v in net.state_dict().items()}, "optimizer": {}}, ck)
    cfg = os.path.join(str(tmp_path), "config.yaml")
    with open(cfg, "w") as f:
        yaml.safe_dump(dict(model=model, data=data, trainer=dict(wandb=False)), f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test_disp.py"), "--config", cfg, "--load_model", ck,
                        "--batch", "2"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    if dataset == "kitti":
        assert "computed error on 2 / 1 missing" in p.stdout, p.stdout
        assert "abs_rel |   sq_rel |" in p.stdout and p.stdout.rstrip().endswith("-> Done!")
    else:
        assert "computed error on 6" in p.stdout and "wrong/all = " in p.stdout and "WHDR = " in p.stdout, p.stdout
