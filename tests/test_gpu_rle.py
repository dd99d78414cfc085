"""Run-length masks on the MI355X: io_rle_decode_u8 (csrc/rle.hip) byte for byte against a NumPy decode written here (a
fill per run -- the kernel searches per pixel), its refusals, and every consumer of ``rle.RLEMasks`` against the same
call on the dense masks: the renderer, the dataset classes (golden items of the reference), the mask rules and the
inference driver."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from helpers import load_golden
from instaorder_amd import _lib, datasets, inference, mask_rules, rle, synthetic

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (61, 83), (33, 130)]
DENSITIES = [0.0, 1.0, 0.5, 0.05]
GUARD, FILL = 48, 0xAB


def ref_encode(mask):
    flat = (np.asarray(mask) != 0).T.reshape(-1).astype(np.int8)          # column-major
    starts = np.flatnonzero(np.diff(np.concatenate([[0], flat])) != 0)      # a leading set pixel starts a run at q = 0
    return np.diff(np.concatenate([[0], starts, [flat.size]])).tolist()


def ref_decode(counts, H, W, value):
    counts = np.asarray(counts, np.int64)
    flat = np.repeat((np.arange(counts.size) & 1) * value, counts).astype(np.uint8)
    assert flat.size == H * W
    return flat.reshape(W, H).T.copy()


def checkerboard_past_lds():
    """the smallest square checkerboard whose run count exceeds the LDS capacity by a table row (= its side) or more"""
    cap = rle.lds_runs()
    for s in range(1, 4096):
        yy, xx = np.mgrid[0:s, 0:s]
        counts = ref_encode((yy + xx) & 1)
        if len(counts) >= cap + s:
            return s, counts
    raise AssertionError("no checkerboard found")


def kernel_cases():
    """(counts, H, W, value, what)"""
    rs = np.random.RandomState(17)
    cases = []
    for k, (H, W) in enumerate(SIZES):
        for j, dens in enumerate(DENSITIES):
            m = rs.rand(H, W) < dens
            cases.append((ref_encode(m), H, W, 7 if (k + j) % 2 else 1, "random %dx%d at %g" % (H, W, dens)))
    m = rs.rand(33, 130) < 0.5
    m[0, 0] = True
    c = ref_encode(m)
    assert c[0] == 0
    cases.append((c, 33, 130, 1, "first pixel set"))
    m = rs.rand(61, 83) < 0.3
    c = ref_encode(m)
    k = next(i for i in range(len(c) // 2, len(c)) if c[i] >= 2)
    c = c[:5] + [0, 0] + c[5:k] + [1, 0, c[k] - 1] + c[k + 1:] + [0, 0, 0]
    cases.append((c, 61, 83, 7, "interior and trailing zero-length runs"))
    cases.append(([0, 0, 0, 5 * 3], 5, 3, 1, "leading zero-length runs, then empty"))
    cases.append(([61 * 83], 61, 83, 1, "single run: empty"))
    cases.append(([0, 61 * 83], 61, 83, 7, "two runs: full"))
    s, c = checkerboard_past_lds()
    cases.append((c, s, s, 1, "checkerboard %dx%d: %d runs, searched in global memory" % (s, s, len(c))))
    return cases


def launch(ends, desc, out, out_bytes=None, ends_count=None, n=None):
    ends_dev = torch.from_numpy(ends.astype(np.uint32)).cuda()
    desc_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).cuda()
    rc = _lib.lib().io_rle_decode_u8(C.c_void_p(ends_dev.data_ptr()), C.c_size_t(ends.size if ends_count is None else ends_count),
                                     C.c_void_p(desc_dev.data_ptr()), C.cast(desc, C.c_void_p), len(desc) if n is None else n,
                                     C.c_void_p(out.data_ptr()), C.c_size_t(out.numel() if out_bytes is None else out_bytes),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_decode_kernel_byte_exact_in_one_launch():
    """masks of different sizes in one launch; values 1 and 7; a first pixel set; zero-length runs; empty and full; widths
    that are no multiple of 4; outputs at offsets of every alignment (16-byte but not 64-byte aligned ones, as the arena
    gives them, and odd ones); a run table longer than the LDS capacity; guard bytes around every output."""
    cases = kernel_cases()
    assert any(len(c[0]) > rle.lds_runs() for c in cases) and any(1 < len(c[0]) <= rle.lds_runs() for c in cases)
    desc = (_lib.RleDesc * len(cases))()
    ends, cursor, e0 = [], 0, 0
    want_align = [16, 48, 16 + 64, 1, 2, 3, 32, 0]            # out_off mod 64, in turn
    for k, (counts, H, W, value, what) in enumerate(cases):
        assert sum(counts) == H * W, what
        cursor += GUARD
        cursor += (want_align[k % len(want_align)] - cursor) % 64
        d = desc[k]
        d.ends_off, d.n_runs, d.H, d.W, d.value, d.out_off = e0, len(counts), H, W, value, cursor
        ends.append(np.cumsum(counts))
        e0 += len(counts)
        cursor += H * W
    total = cursor + GUARD
    assert any(desc[k].out_off % 64 == 16 for k in range(len(cases)))
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 64 == 0
    assert launch(np.concatenate(ends), desc, out) == 0, _lib.last_error()
    got = out.cpu().numpy()
    expect = np.full(total, FILL, np.uint8)
    for k, (counts, H, W, value, what) in enumerate(cases):
        o = desc[k].out_off
        ref = ref_decode(counts, H, W, value)
        assert np.array_equal(got[o:o + H * W].reshape(H, W), ref), what
        expect[o:o + H * W] = ref.reshape(-1)
    assert np.array_equal(got, expect), "a guard byte was written"


def test_decode_wrapper_and_profile_class():
    """rle.decode == to_dense(); the launch is timed under its own class with bytes = table bytes + pixels"""
    m = (np.random.RandomState(2).rand(5, 37, 29) < 0.4).astype(np.uint8)
    r = rle.RLEMasks.from_dense(m).with_values([1, 2, 3, 250, 255])
    L = _lib.lib()
    L.io_prof_begin_ex(0)
    got = rle.decode(r, "cuda:0")
    ent = (_lib.ProfEntry * 32)()
    n = L.io_prof_end(ent, 32)
    assert np.array_equal(got.cpu().numpy(), r.to_dense())
    mine = [e for e in ent[:n] if e.name == b"rle_decode"]
    assert len(mine) == 1 and mine[0].launches == 1
    assert mine[0].bytes == 4.0 * r.ends()[0].size + m.size


def test_entry_point_refusals():
    """a table past ends_count, an output past out_bytes, n_runs == 0, value == 256: IO_ERR_SHAPE, no launch, `out` as it was"""
    H, W = 5, 3
    counts = [4, 6, 5]
    ends = np.cumsum(counts)
    out = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    L = _lib.lib()

    def call(ends_count=None, out_bytes=None, **kw):
        d = (_lib.RleDesc * 1)()
        base = dict(ends_off=0, n_runs=3, H=H, W=W, value=1, out_off=16)
        base.update(kw)
        for k, v in base.items():
            setattr(d[0], k, v)
        return launch(ends, d, out, out_bytes=out_bytes, ends_count=ends_count)

    L.io_prof_begin_ex(0)
    assert call(ends_off=1) == -1 and "table" in _lib.last_error()                   # entries 1..3 of a 3-entry buffer
    assert call(ends_count=2) == -1
    assert call(out_off=256 - 14) == -1 and "output" in _lib.last_error()            # 15 bytes from 242: one too many
    assert call(out_bytes=30) == -1
    assert call(n_runs=0) == -1 and "n_runs" in _lib.last_error()
    assert call(value=256) == -1 and "value" in _lib.last_error()
    assert call(value=-1) == -1 and call(H=0) == -1 and call(ends_off=-1) == -1 and call(out_off=-1) == -1
    ent = (_lib.ProfEntry * 32)()
    assert L.io_prof_end(ent, 32) == 0, "a refused call launched something"
    assert bool((out == FILL).all())
    assert call(out_off=256 - 15) == 0                       # the same call, inside by one byte, is taken
    got = out.cpu().numpy()
    assert np.array_equal(got[241:256].reshape(H, W), ref_decode(counts, H, W, 1)) and (got[:241] == FILL).all()


def test_renderer_rle_equals_dense_bit_for_bit():
    """the items and images of the oracle test at S = 32: run-length masks (one of them category-valued) render as the
    dense masks do, also in a batch that mixes both kinds, without the image, and on reused staging buffers"""
    S = 32
    rng = np.random.RandomState(5 + S)
    images = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in [(61, 83), (120, 47), (33, 33)]]
    masks = [(rng.rand(3, im.shape[0], im.shape[1]) < 0.4).astype(np.uint8) for im in images]
    masks[1][2] *= 7                                    # use_category: mask values are category ids
    items = []
    for ii, im in enumerate(images):
        H, W = im.shape[:2]
        boxes = [(0, 0, W, H), (-9, -13, W + 20, H + 30), (W // 3, H // 4, 11, 11), (W - 5, H - 6, 40, 40),
                 (-30, 5, 25, 25), (2, 3, 3 * S, 3 * S), (5, 5, 7, 19), (-500, -500, 10, 10), (1, 1, 1, 1)]
        for k, box in enumerate(boxes):
            items.append((ii, k % 3, (k + 1) % 3, box, 1 + (k + ii) % 2, bool(k % 2)))
            items.append((ii, (k + 2) % 3, k % 3, box, 2 - (k + ii) % 2, not bool(k % 2)))
            items.append((ii, k % 3, (k + 2) % 3, box, 3, bool((k + ii) % 2)))       # cubic on the float64 image
    rmasks = [rle.RLEMasks.from_dense(m != 0).with_values(m.reshape(3, -1).max(axis=1)) for m in masks]
    assert list(rmasks[1].values) == [1, 1, 7]
    want = [t.cpu().numpy() for t in datasets.PairRenderer(S, MEAN, STD).render(images, masks, items)]
    r = datasets.PairRenderer(S, MEAN, STD)
    for name, mm in (("rle", rmasks), ("mixed", [masks[0], rmasks[1], rmasks[2]])):
        got = r.render(images, mm, items)
        for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
            assert np.array_equal(g.cpu().numpy(), w), (name, plane)
    up = r.last_upload
    assert up["images"] == sum(im.size for im in images) and up["masks"] == masks[0].size + 4 * sum(
        rmasks[i].ends()[0].size for i in (1, 2))
    rgb0, m1b, m2b = r.render(images, rmasks, items[:5], load_rgb=False)
    assert float(rgb0.abs().max()) == 0.0
    assert np.array_equal(m1b.cpu().numpy(), want[1][:5]) and np.array_equal(m2b.cpu().numpy(), want[2][:5])
    assert r.last_upload["images"] == 0
    rgb2, m1c, _ = r.render(images, rmasks, items[7:19])                  # both staging buffers have been used by now
    assert np.array_equal(rgb2.cpu().numpy(), want[0][7:19]) and np.array_equal(m1c.cpu().numpy(), want[1][7:19])


@pytest.mark.parametrize("k", range(6))
def test_batches_over_an_rle_reader_equal_reference_dataset_items(k):
    """batch() over RLEReader(SyntheticReader) == the golden items of the reference's dataset classes, all six variants"""
    z = load_golden("dataset_items")
    cfg = json.loads(str(z["config_json"]))
    name, kind, algo, mode, phase, seed = str(z["variants"][k]).split("|")
    cfg = dict(cfg, patch_or_image=mode)
    rd = rle.RLEReader(synthetic.SyntheticReader(int(z["reader_seed"])))
    cls = {"occ": datasets.SupOcclusionOrderBatches, "depth_occ": datasets.SupDepthOccOrderBatches,
           "depth": datasets.SupDepthOrderBatches}[kind]
    ds = cls(cfg, phase, algo, rd, rd.load_image)
    np.random.seed(int(seed))
    n = z[name + "_f0"].shape[0]
    out = ds.batch(range(n))
    assert len(out) == {"occ": 4, "depth_occ": 7, "depth": 6}[kind]
    for f, t in enumerate(out):
        assert t.is_cuda
        g = z["%s_f%d" % (name, f)]
        assert np.array_equal(t.cpu().numpy().astype(g.dtype), g), (name, f)


@pytest.fixture(scope="module")
def scene():
    sc = synthetic.SyntheticReader(3).scenes[0]
    return sc, rle.RLEMasks.from_dense(sc["modal"])


def test_mask_rules_pair_relations(scene):
    sc, rm = scene
    want, got = mask_rules.pair_relations(sc["modal"]), mask_rules.pair_relations(rm)
    assert sorted(want) == sorted(got)
    for key in want:
        assert np.array_equal(want[key], got[key]), key
    want, got = mask_rules.pair_relations(sc["modal"], sc["modal"]), mask_rules.pair_relations(rm, rm)
    assert np.array_equal(want["inter"], got["inter"])
    assert np.array_equal(mask_rules.infer_gt_order(sc["modal"], sc["modal"]), mask_rules.infer_gt_order(rm, rm))
    assert np.array_equal(mask_rules.infer_occ_order_area(sc["modal"]), mask_rules.infer_occ_order_area(rm))
    assert np.array_equal(mask_rules.infer_depth_order_yaxis(sc["modal"]), mask_rules.infer_depth_order_yaxis(rm))


def test_mask_rules_select_pairs_nbor(scene):
    sc, rm = scene
    want = mask_rules.select_pairs(sc["modal"], "nbor")
    assert want == inference.select_pairs(sc["modal"], "nbor") and len(want) > 0
    assert mask_rules.select_pairs(rm, "nbor") == want


def test_mask_rules_depth_orders_from_disp(scene):
    sc, rm = scene
    n, H, W = sc["modal"].shape
    disp = torch.from_numpy(np.random.RandomState(8).rand(H, W).astype(np.float32) + 0.1).cuda()
    pairs = inference.upper_pairs(n)
    for method in ("median", "mean"):
        want = mask_rules.depth_orders_from_disp(disp, sc["modal"], pairs, method)
        assert np.array_equal(mask_rules.depth_orders_from_disp(disp, rm, pairs, method), want), method
        assert want.any()


@pytest.fixture(scope="module")
def net():
    import instaorder_amd as ia
    params = dict(algo="InstaOrderNet_o", lr=1e-3, weight_decay=1e-4, optim="SGD", use_rgb=True,
                  backbone_arch="resnet50_cls", backbone_param=dict(in_channels=5, num_classes=2))
    m = ia.InstaOrderNet_o(params, dist_model=False)
    m.switch_to("eval")
    return m


@pytest.mark.parametrize("mode", ["patch", "image", "resize", "orig"])
def test_infer_order_sup_occ_rle_equals_dense(net, mode):
    """the same order matrix from run-length masks as from dense ones, with the device rules (the masks never exist on the
    host) and with the host rules (decoded once)"""
    sc = synthetic.SyntheticReader(9, n_images=4, n_inst=4, empty_every=0).scenes[1]
    rm = rle.RLEMasks.from_dense(sc["modal"])
    S = 64
    for pairs in ("all", "nbor"):
        want = inference.infer_order_sup_occ(net, sc["image"], sc["modal"], sc["bboxes"], pairs, "InstaOrderNet_o", mode, S)
        for rules in ("device", "host"):
            got = inference.infer_order_sup_occ(net, sc["image"], rm, sc["bboxes"], pairs, "InstaOrderNet_o", mode, S,
                                                mask_rules=rules)
            assert np.array_equal(got, want), (pairs, rules)
    assert want.shape == (4, 4)


def test_evaluate_rle_reader_equals_dense_reader(net):
    """evaluate() over an RLEReader: the model-free 'area' rule with inferred ground truth (modal and amodal masks both
    run-length, category-valued) and the network method in 'patch' mode, with the device rules and with the host rules,
    give the orders and metrics of the dense reader"""
    from instaorder_amd import evaluate
    rd = synthetic.SyntheticReader(5, n_images=3, n_inst=6, empty_every=0)

    class Reader(object):                  # the KINS / COCOA form: amodal masks come with the instances
        def __init__(self, encode):
            self.encode = encode

        def get_image_length(self):
            return rd.get_image_length()

        def get_image_instances(self, i, with_gt=False):
            modal, cat, bb, _, fn = rd.get_image_instances(i, with_gt)
            am = modal.copy()
            am[:, ::3] = 1
            if self.encode:
                modal, am = rle.RLEMasks.from_dense(modal), rle.RLEMasks.from_dense(am)
            return modal, cat, bb, am, fn

    cfg = dict(trainval_dataset="SupOcclusionOrderDataset", patch_or_image="patch", input_size=64, dataset="COCOA",
               enlarge_box=3.0, use_category=True)
    want = evaluate.evaluate(None, Reader(False), rd.load_image, cfg, "area", gt_ordering="infer", return_orders=True)
    for rules in ("device", "host"):
        got = evaluate.evaluate(None, Reader(True), rd.load_image, cfg, "area", gt_ordering="infer", return_orders=True,
                                mask_rules=rules)
        for key in ("recall", "precision", "f1"):
            assert want[key] == got[key], (rules, key)
        for i in range(3):
            assert np.array_equal(want["orders"][i][0], got["orders"][i][0]), (rules, i)
    z = load_golden("tester")
    ncfg = dict(json.loads(str(z["data_cfg_json"])), trainval_dataset="SupOcclusionOrderDataset", patch_or_image="patch",
                input_size=64)
    rd4 = synthetic.SyntheticReader(9, n_images=4, n_inst=4, empty_every=0)
    want = evaluate.evaluate(net, rd4, rd4.load_image, ncfg, "InstaOrderNet_o", pairs="nbor", return_orders=True)
    for rules in ("device", "host"):
        got = evaluate.evaluate(net, rle.RLEReader(rd4), rd4.load_image, ncfg, "InstaOrderNet_o", pairs="nbor",
                                return_orders=True, mask_rules=rules)
        assert want["f1"] == got["f1"]
        for i in range(4):
            assert np.array_equal(want["orders"][i][0], got["orders"][i][0]), (rules, i)


def test_infer_order_sup_depth_midas_rle_equals_dense(scene):
    """the disparity-selected depth orders ('resize' mode, a stand-in disparity model): run-length masks with the device
    rules and with the host rules against dense masks"""
    sc, rm = scene

    class Disp(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([0.7, 0.2, 0.4]).view(1, 3, 1, 1))

        def forward(self, x):
            return (x * self.w).sum(1).abs() + 0.5

    model = Disp().cuda()
    want, _ = inference.infer_order_sup_depth(model, sc["image"], sc["modal"], sc["bboxes"], "all", "midas_pretrained",
                                              "resize", 64, "median")
    for rules in ("device", "host"):
        got, _ = inference.infer_order_sup_depth(model, sc["image"], rm, sc["bboxes"], "all", "midas_pretrained", "resize",
                                                 64, "median", mask_rules=rules)
        assert np.array_equal(got, want), rules
    assert want.any()
