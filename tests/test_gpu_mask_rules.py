"""Device mask rules on the MI355X (instaorder_amd.mask_rules, csrc/mask_rules.hip) against the unchanged host functions
of instaorder_amd.inference, NumPy restatements and the reference goldens: packing and pair counts bit for bit, the
'nbor' pair selection, the heuristics and infer_gt_order, evaluate(mask_rules='device'), the disparity-selected depth
orders (exact order statistics against torch.quantile / torch.median on the device), a large image and the ABI's error
paths."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import GOLDEN, synthetic
from instaorder_amd import _lib, evaluate, inference, mask_rules

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _rand_masks(rs, n, H, W, values=(1,)):
    """n masks: random blobs, one empty, one full (touching all four borders), one border frame; values from ``values``"""
    m = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        kind = i % 5
        v = values[i % len(values)]
        if kind == 0:
            m[i] = (rs.rand(H, W) < 0.3) * v
        elif kind == 1:
            y0, x0 = rs.randint(0, H), rs.randint(0, W)
            m[i, y0:y0 + rs.randint(1, H + 1), x0:x0 + rs.randint(1, W + 1)] = v
        elif kind == 2:
            m[i] = v                                           # full: touches every border
        elif kind == 3:
            m[i, 0, :] = m[i, -1, :] = m[i, :, 0] = m[i, :, -1] = v
        # kind 4: empty
    return m


def _np_dilate(a):
    """one step of the 3x3 cross over the last two axes (rows, columns) of a bool stack"""
    d = a.copy()
    d[..., 1:, :] |= a[..., :-1, :]
    d[..., :-1, :] |= a[..., 1:, :]
    d[..., :, 1:] |= a[..., :, :-1]
    d[..., :, :-1] |= a[..., :, 1:]
    return d


def _np_bits(b):
    """bool [n, H, W] -> uint32 [n, H, ceil(W/32)] with pixel x at bit x % 32 of word x / 32"""
    n, H, W = b.shape
    Wq = (W + 31) // 32
    pad = np.zeros((n, H, Wq * 32), bool)
    pad[:, :, :W] = b
    return np.packbits(pad, axis=-1, bitorder="little").view("<u4").reshape(n, H, Wq)


def _count_ref(p, q):
    a = p.reshape(p.shape[0], -1).astype(np.float64)
    b = q.reshape(q.shape[0], -1).astype(np.float64)
    return (a @ b.T).astype(np.int64)


CASES = [(W, H, n) for W in (1, 31, 32, 33, 95, 640) for H in (1, 2, 17, 480) for n in (1, 2, 7, 64)
         if W * H * n <= 640 * 480 * 7 or (W, H, n) == (640, 480, 64)]


@pytest.mark.parametrize("W,H,n", CASES)
def test_pack_and_counts_bit_exact(W, H, n):
    rs = np.random.RandomState(W * 1000 + H * 10 + n)
    m = _rand_masks(rs, n, H, W, values=(1, 3) if n > 1 else (1,))
    md = torch.from_numpy(m).to(DEV)
    stats = torch.empty((n, 4), dtype=torch.int64, device=DEV)
    eq1, nz = m == 1, m != 0
    dil = mask_rules.pack(md, 1, dilate=True, stats=stats)
    one = mask_rules.pack(md, 1)
    nzb = mask_rules.pack(md, 0)
    nzd = mask_rules.pack(md, 0, dilate=True)
    for got, want in ((dil, _np_dilate(eq1)), (one, eq1), (nzb, nz), (nzd, _np_dilate(nz))):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), _np_bits(want))
    rows = np.arange(H, dtype=np.int64)[None, :, None]
    st = np.stack([m.reshape(n, -1).astype(np.int64).sum(1), eq1.reshape(n, -1).sum(1),
                   (eq1 * rows).reshape(n, -1).sum(1), nz.reshape(n, -1).sum(1)], 1)
    assert np.array_equal(stats.cpu().numpy(), st)
    assert np.array_equal(mask_rules.pair_counts(dil, nzb, W).cpu().numpy(), _count_ref(_np_dilate(eq1), nz))
    # rectangular count matrices (n_p != n_q)
    k = max(1, n // 3)
    assert np.array_equal(mask_rules.pair_counts(one[:k], nzb, W).cpu().numpy(), _count_ref(eq1[:k], nz))


def test_touch_equals_bordering_and_select_pairs_equal_host():
    rs = np.random.RandomState(7)
    for seed in range(4):
        rd = synthetic.SyntheticReader(40 + seed, n_images=3, n_inst=9, empty_every=2)
        for sc in rd.scenes:
            m = sc["modal"]
            r = mask_rules.pair_relations(m)
            n = m.shape[0]
            want = np.array([[inference.bordering(m[i], m[j]) for j in range(n)] for i in range(n)], bool).reshape(n, n)
            assert np.array_equal(r["touch"], want)
            for pairs in ("all", "nbor"):
                assert mask_rules.select_pairs(m, pairs) == inference.select_pairs(m, pairs)
                assert mask_rules.select_pairs(torch.from_numpy(m).to(DEV).float(), pairs) == \
                    inference.select_pairs(m, pairs)
    m = _rand_masks(rs, 12, 37, 41, values=(1, 2, 3))              # category-valued: only '== 1' is dilated
    r = mask_rules.pair_relations(m)
    want = np.array([[inference.bordering(m[i], m[j]) for j in range(12)] for i in range(12)], bool)
    assert np.array_equal(r["touch"], want)
    assert np.array_equal(r["area"], m.reshape(12, -1).astype(np.int64).sum(1))


def test_heuristics_and_gt_order_equal_reference_golden():
    z = np.load(os.path.join(GOLDEN, "heuristics.npz"))
    rd = synthetic.SyntheticReader(88, n_images=4, n_inst=6, empty_every=0)
    for k, sc in enumerate(rd.scenes):
        m = sc["modal"]
        got = {"occ_area_s": mask_rules.infer_occ_order_area(m, "smaller"),
               "occ_area_l": mask_rules.infer_occ_order_area(m, "larger"),
               "occ_y_lo": mask_rules.infer_occ_order_yaxis(m, "lower"),
               "occ_y_hi": mask_rules.infer_occ_order_yaxis(m, "higher"),
               "dep_area_s": mask_rules.infer_depth_order_area(m, "smaller"),
               "dep_area_l": mask_rules.infer_depth_order_area(m, "larger"),
               "dep_y_lo": mask_rules.infer_depth_order_yaxis(m, "lower"),
               "dep_y_hi": mask_rules.infer_depth_order_yaxis(m, "higher"),
               "gt": mask_rules.infer_gt_order(m, z["amodal_%d" % k])}
        for name, v in got.items():
            assert v.dtype == np.int64
            assert np.array_equal(v, z["%s_%d" % (name, k)]), (name, k)


def test_heuristics_equal_host_with_empty_and_category_masks():
    """ties, masks without a '== 1' pixel (NaN centre) and category values: the host functions are the definition"""
    rs = np.random.RandomState(11)
    for t in range(6):
        m = _rand_masks(rs, 8 + t, 30 + t, 45, values=(1, 3) if t % 2 else (1,))
        am = np.maximum(m, (rs.rand(*m.shape) < 0.1).astype(np.uint8))
        for f, a in (("infer_occ_order_area", "smaller"), ("infer_occ_order_yaxis", "lower"),
                     ("infer_occ_order_yaxis", "higher"), ("infer_depth_order_area", "larger"),
                     ("infer_depth_order_yaxis", "lower"), ("infer_depth_order_yaxis", "higher")):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)          # the host's mean of an empty selection
                want = getattr(inference, f)(m, a)
            assert np.array_equal(getattr(mask_rules, f)(m, a), want), (f, a, t)
        assert np.array_equal(mask_rules.infer_gt_order(m, am), inference.infer_gt_order(m, am)), t


@pytest.mark.parametrize("k", range(4))
def test_evaluate_device_equals_reference_tester(k):
    z = np.load(os.path.join(GOLDEN, "tester.npz"))
    cfg = json.loads(str(z["data_cfg_json"]))
    name, kind, method, mode, algo = str(z["scenarios"][k]).split("|")
    S, seed, rseed, warm = [int(v) for v in z["meta"]]
    rd = synthetic.SyntheticReader(rseed, n_images=4, n_inst=5, empty_every=0)
    res = evaluate.evaluate(None, rd, rd.load_image, dict(cfg, trainval_dataset=kind, patch_or_image=mode), method,
                            return_orders=True, mask_rules="device")
    for i in range(4):
        occ, dep = res["orders"][i]
        assert np.array_equal(occ if dep is None else dep, z["%s_pred_%d" % (name, i)])
    if kind == "SupOcclusionOrderDataset":
        for key in ("recall", "precision", "f1"):
            assert abs(res[key] - float(z["%s_log_val.%s" % (name, key)])) < 1e-9
    else:
        for key in evaluate.WHDR_KEYS:
            ovl, eq = key.split("_")
            assert abs(res["WHDR_" + key] - float(z["%s_log_val_%s.WHDR_%s" % (name, ovl, eq)])) < 1e-9


def test_evaluate_gt_ordering_infer_device_equals_host():
    rd = synthetic.SyntheticReader(5, n_images=3, n_inst=6, empty_every=0)

    class Reader(object):                  # the KINS / COCOA form: amodal masks come with the instances
        def get_image_length(self):
            return rd.get_image_length()

        def get_image_instances(self, i, with_gt=False):
            modal, cat, bb, _, fn = rd.get_image_instances(i, with_gt)
            am = modal.copy()
            am[:, ::3] = 1
            return modal, cat, bb, am, fn

    cfg = dict(trainval_dataset="SupOcclusionOrderDataset", patch_or_image="patch", input_size=64, dataset="COCOA",
               enlarge_box=3.0)
    a = evaluate.evaluate(None, Reader(), rd.load_image, cfg, "area", gt_ordering="infer", return_orders=True)
    b = evaluate.evaluate(None, Reader(), rd.load_image, cfg, "area", gt_ordering="infer", return_orders=True,
                          mask_rules="device")
    for key in ("recall", "precision", "f1"):
        assert a[key] == b[key]
    for i in range(3):
        assert np.array_equal(a["orders"][i][0], b["orders"][i][0])


# ---- disparity selection -------------------------------------------------------------------------------------------------
def _disp_case(rs, H, W, n, tied=False):
    disp = (rs.rand(H, W).astype(np.float32) * 3 + np.float32(0.05))
    if tied:
        disp = (rs.randint(0, 6, size=(H, W)) / np.float32(4) + np.float32(0.25)).astype(np.float32)
    m = (rs.rand(n, H, W) < rs.uniform(0.02, 0.6, size=(n, 1, 1))).astype(np.uint8)
    m[0] = 0
    m[0].reshape(-1)[rs.randint(H * W)] = 1                  # k = 1
    m[1] = 0
    m[1].reshape(-1)[rs.choice(H * W, 2, replace=False)] = 1   # k = 2
    m[2] = 0
    m[2].reshape(-1)[rs.choice(H * W, 3, replace=False)] = 1   # k = 3
    m[3] = 1                                                   # everything
    m[4] *= 3                                                  # a category value
    return torch.from_numpy(disp).to(DEV), m


@pytest.mark.parametrize("H,W,n,tied", [(48, 64, 9, False), (48, 64, 9, True), (375, 1242, 6, False), (17, 95, 12, True)])
def test_instance_statistics_equal_torch(H, W, n, tied):
    rs = np.random.RandomState(H + W + n + tied)
    disp, m = _disp_case(rs, H, W, n, tied)
    md = torch.from_numpy(m).to(DEV)
    depth = 1 / (disp + 1e-6)
    for method in (0, 1):
        val, lo, hi, k = (t.cpu().numpy().copy() for t in mask_rules.instance_depth_select(disp, md, method))
        for i in range(n):
            v = depth[md[i].bool()]
            assert k[i] == v.numel()
            ql, qh = torch.quantile(v, 0.05), torch.quantile(v, 0.95)
            assert lo[i] == float(ql) and hi[i] == float(qh), (i, lo[i], float(ql), hi[i], float(qh))
            c = torch.clip(v, ql, qh)
            if method == 1:
                assert val[i] == float(torch.median(c)), (i, val[i], float(torch.median(c)))
            else:
                ref = float(torch.mean(c.double()))
                assert abs(val[i] - ref) <= 1e-6 * abs(ref), (i, val[i], ref)


def _host_orders(disp, masks, pairs, method):
    n = masks.shape[0]
    order = np.zeros((n, n), dtype=np.int64)
    for i, j in pairs:
        a = inference.net_forward_midas_pretrained(disp, masks[i], masks[j], method)
        order[i, j], order[j, i] = {0: (1, 0), 1: (0, 1), 2: (2, 2)}[a]
    return order


@pytest.mark.parametrize("method", ["median", "mean"])
def test_depth_orders_equal_host_loop(method):
    rs = np.random.RandomState(3)
    for H, W, n, tied in ((48, 64, 9, False), (40, 33, 8, True)):
        disp, m = _disp_case(rs, H, W, n, tied)
        pairs = inference.upper_pairs(n)
        want = _host_orders(disp, m, pairs, method)
        assert np.array_equal(mask_rules.depth_orders_from_disp(disp, m, pairs, method), want)
        assert np.array_equal(mask_rules.depth_orders_from_disp(disp[None, None], torch.from_numpy(m).to(DEV).float(),
                                                                pairs, method), want)
        sub = pairs[::3]
        assert np.array_equal(mask_rules.depth_orders_from_disp(disp, m, sub, method), _host_orders(disp, m, sub, method))
    # a constant map: every selected pair is equal
    c = torch.full((20, 30), 0.5, device=DEV)
    m = (rs.rand(5, 20, 30) < 0.4).astype(np.uint8)
    o = mask_rules.depth_orders_from_disp(c, m, inference.upper_pairs(5), method)
    assert np.array_equal(o, 2 * (1 - np.eye(5, dtype=np.int64)))


def test_empty_instance_raises_only_inside_a_selected_pair():
    rs = np.random.RandomState(4)
    disp = torch.from_numpy(rs.rand(20, 30).astype(np.float32) + 0.1).to(DEV)
    m = (rs.rand(4, 20, 30) < 0.4).astype(np.uint8)
    m[2] = 0
    with pytest.raises(RuntimeError):
        mask_rules.depth_orders_from_disp(disp, m, [(0, 1), (1, 2)], "median")
    with pytest.raises(RuntimeError):
        inference.net_forward_midas_pretrained(disp, m[1], m[2], "median")          # the host path raises too
    pairs = [(0, 1), (0, 3), (1, 3)]
    assert np.array_equal(mask_rules.depth_orders_from_disp(disp, m, pairs, "mean"), _host_orders(disp, m, pairs, "mean"))


class _Midas(torch.nn.Module):
    """stands in for the bare MidasNet of midas_pretrained: disparity = a fixed function of the image"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.7, -0.2, 0.4], device=DEV))

    def forward(self, rgb):
        return (rgb * self.w[None, :, None, None]).sum(1, keepdim=True).abs() + 0.1


@pytest.mark.parametrize("mode", ["image", "resize"])
@pytest.mark.parametrize("pairs", ["all", "nbor"])
@pytest.mark.parametrize("method", ["median", "mean"])
def test_infer_order_sup_depth_midas_pretrained_device_equals_host(mode, pairs, method):
    S = 64
    rs = np.random.RandomState(21)
    image = rs.randint(0, 256, size=(S, S, 3)).astype(np.uint8) if mode == "image" else \
        rs.randint(0, 256, size=(50, 70, 3)).astype(np.uint8)
    hh, ww = image.shape[:2]
    inmodal = np.zeros((7, hh, ww), np.uint8)
    for i in range(7):
        y, x = rs.randint(0, hh - 8), rs.randint(0, ww - 8)
        inmodal[i, y:y + rs.randint(6, 30), x:x + rs.randint(6, 30)] = 1
    net = _Midas()
    a, ca = inference.infer_order_sup_depth(net, image, inmodal, None, pairs, "midas_pretrained", mode, S, method)
    b, cb = inference.infer_order_sup_depth(net, image, inmodal, None, pairs, "midas_pretrained", mode, S, method,
                                            mask_rules="device")
    assert np.array_equal(a, b)
    assert torch.equal(ca, cb)
    if pairs == "all":
        assert (a != 0).any()


def test_large_image_against_host_sample():
    rs = np.random.RandomState(200)
    n, H, W = 200, 375, 1242
    m = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        y, x = rs.randint(0, H), rs.randint(0, W)
        m[i, y:y + rs.randint(1, 120), x:x + rs.randint(1, 200)] = 1 if i % 7 else 2
    am = np.maximum(m, np.roll(m, 3, axis=2))
    r = mask_rules.pair_relations(m, am)
    assert np.array_equal(r["area"], m.reshape(n, -1).astype(np.int64).sum(1))
    for _ in range(300):
        i, j = rs.randint(n), rs.randint(n)
        assert r["touch"][i, j] == inference.bordering(m[i], m[j]), (i, j)
        assert r["inter"][i, j] == int(((m[i] == 1) & (am[j] == 1)).sum()), (i, j)
    disp = torch.from_numpy(rs.rand(H, W).astype(np.float32) + 0.05).to(DEV)
    md = torch.from_numpy(m).to(DEV)
    val, lo, hi, k = (t.cpu().numpy().copy() for t in mask_rules.instance_depth_select(disp, md, 1))
    depth = 1 / (disp + 1e-6)
    for i in rs.choice(n, 12, replace=False):
        v = depth[md[i].bool()]
        ql, qh = torch.quantile(v, 0.05), torch.quantile(v, 0.95)
        assert (k[i], lo[i], hi[i], val[i]) == (v.numel(), float(ql), float(qh), float(torch.median(torch.clip(v, ql, qh))))
    sample = [tuple(int(v) for v in rs.choice(n, 2, replace=False)) for _ in range(40)]
    for method in ("median", "mean"):
        assert np.array_equal(mask_rules.depth_orders_from_disp(disp, m, sample, method),
                              _host_orders(disp, m, sample, method))


def test_abi_error_paths_launch_nothing():
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    m = torch.ones((2, 8, 40), dtype=torch.uint8, device=DEV)
    bits = torch.full((2, 8, 2), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((2, 4), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
    disp = torch.ones((8, 40), device=DEV)
    out = torch.full((4, 2), -7.0, device=DEV)
    nws = lib.io_instance_depth_select_workspace_bytes(2, 8, 40)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    SHAPE, WORKSPACE = -1, -2
    p, b, s, c = m.data_ptr(), bits.data_ptr(), stats.data_ptr(), counts.data_ptr()
    calls = [
        (SHAPE, lambda: lib.io_mask_pack(p, 0, 8, 40, 1, 1, b, s, st)),
        (SHAPE, lambda: lib.io_mask_pack(p, 2, 0, 40, 1, 1, b, s, st)),
        (SHAPE, lambda: lib.io_mask_pack(p, 2, 8, -3, 1, 1, b, s, st)),
        (SHAPE, lambda: lib.io_mask_pack(p, 2, 8, 40, 5, 1, b, s, st)),
        (SHAPE, lambda: lib.io_mask_pack(None, 2, 8, 40, 1, 1, b, s, st)),
        (SHAPE, lambda: lib.io_mask_pack(p, 2, 8, 40, 1, 1, None, s, st)),
        (SHAPE, lambda: lib.io_mask_pack(p, 2, 1 << 16, 1 << 15, 1, 1, b, s, st)),       # H * W >= 2^31
        (SHAPE, lambda: lib.io_mask_pair_counts(b, 0, b, 2, 8, 40, c, st)),
        (SHAPE, lambda: lib.io_mask_pair_counts(b, 2, b, 0, 8, 40, c, st)),
        (SHAPE, lambda: lib.io_mask_pair_counts(b, 2, b, 2, 0, 40, c, st)),
        (SHAPE, lambda: lib.io_mask_pair_counts(b, 2, b, 2, 8, 0, c, st)),
        (SHAPE, lambda: lib.io_mask_pair_counts(None, 2, b, 2, 8, 40, c, st)),
        (SHAPE, lambda: lib.io_mask_pair_counts(b, 2, b, 2, 8, 40, None, st)),
        (SHAPE, lambda: lib.io_mask_pair_counts(b, 70000, b, 2, 8, 40, c, st)),
        (SHAPE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 8, 40, p, 0, 1, out.data_ptr(), None, None, None,
                                                     ws.data_ptr(), nws, st)),
        (SHAPE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 0, 40, p, 2, 1, out.data_ptr(), None, None, None,
                                                     ws.data_ptr(), nws, st)),
        (SHAPE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 8, -1, p, 2, 1, out.data_ptr(), None, None, None,
                                                     ws.data_ptr(), nws, st)),
        (SHAPE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 8, 40, p, 2, 7, out.data_ptr(), None, None, None,
                                                     ws.data_ptr(), nws, st)),
        (SHAPE, lambda: lib.io_instance_depth_select(None, 8, 40, p, 2, 1, out.data_ptr(), None, None, None,
                                                     ws.data_ptr(), nws, st)),
        (SHAPE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 8, 40, None, 2, 1, out.data_ptr(), None, None, None,
                                                     ws.data_ptr(), nws, st)),
        (SHAPE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 8, 40, p, 2, 1, None, None, None, None,
                                                     ws.data_ptr(), nws, st)),
        (WORKSPACE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 8, 40, p, 2, 1, out.data_ptr(), None, None, None,
                                                         ws.data_ptr(), nws - 1, st)),
        (WORKSPACE, lambda: lib.io_instance_depth_select(disp.data_ptr(), 8, 40, p, 2, 1, out.data_ptr(), None, None, None,
                                                         None, nws, st)),
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, k
        assert _lib.last_error()
    torch.cuda.synchronize()
    assert (bits == -7).all() and (stats == -7).all() and (counts == -7).all() and (out == -7).all()
