"""COCO polygon masks on the MI355X: io_poly_fill_u8 (csrc/poly.hip) byte for byte against the sequential oracle of
tests/test_poly_cpu.py (walk, positions, sort, run lengths, fill -- the kernels toggle, scan and gather bit planes), its
refusals, and every consumer of ``poly.PolyMasks`` against the same call on ``to_dense()``: ``decode``, the renderer, a
dataset class, the mask rules and the inference driver."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from helpers import load_golden
from instaorder_amd import _lib, datasets, inference, mask_rules, poly, rle, synthetic
from test_poly_cpu import IMAGES, VECTORS, oracle_mask, random_instances, random_part

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
GUARD, FILL = 48, 0xAB


def kernel_cases():
    """(parts, H, W, value, what)"""
    cases = []
    for k, (H, W) in enumerate(IMAGES + [(33, 130)]):
        for i, parts in enumerate(random_instances(7 + k, H, W, 12)):       # 0..3 parts, 1..8 vertices, every style
            cases.append((parts, H, W, 7 if (k + i) % 2 else 1, "random %dx%d #%d" % (H, W, i)))
        cases.append(([[-1, -1, W + 1, -1, W + 1, H + 1, -1, H + 1]], H, W, 7, "the whole %dx%d image" % (H, W)))
        rs = np.random.RandomState(70 + k)
        for i, style in enumerate(("int", "half", "cent", "cent")):          # polygons that cross the image
            cases.append(([random_part(rs, H, W, style, k=5 + i)], H, W, 1 if i % 2 else 7, "%s %dx%d" % (style, H, W)))
    for H, W, flat, _, _ in VECTORS:
        cases.append(([flat], H, W, 1, "fixed vector %dx%d" % (H, W)))
    # a bit plane of more than one pass of the scan block (and of more than two), in a width that is no multiple of 4
    H = 97
    for passes in (1, 2):
        W = (passes * poly.scan_words() * 32) // H + 6
        assert H * W > passes * poly.scan_words() * 32 and W % 4
        rs = np.random.RandomState(40 + passes)
        parts = [random_part(rs, H, W, "cent", k=8), random_part(rs, H, W, "half", k=5),
                 [W - 9.5, H - 7.25, W + 3, H - 6, W - 2.5, H + 4]]            # the last columns and rows
        cases.append((parts, H, W, 1 + 6 * (passes - 1), "%dx%d: more than %d scan passes" % (H, W, passes)))
    return cases


def upload(a):
    return torch.from_numpy(np.frombuffer(a, dtype=np.uint8).copy() if not isinstance(a, np.ndarray) else a.copy()).cuda()


def launch(t_verts, t_parts, t_n_parts, t_masks, t_out, t_ws, **over):
    """io_poly_fill_u8 with device copies of the tables as given; ``over`` replaces single arguments of the call"""
    keep = [upload(t_verts.view(np.uint8).reshape(-1) if t_verts.size else np.zeros(16, np.uint8)),
            upload(over.pop("parts_dev_table", t_parts)), upload(over.pop("masks_dev_table", t_masks))]
    a = dict(verts=keep[0].data_ptr(), n_verts=t_verts.shape[0], parts_dev=keep[1].data_ptr(),
             parts_host=C.cast(t_parts, C.c_void_p), n_parts=t_n_parts, masks_dev=keep[2].data_ptr(),
             masks_host=C.cast(t_masks, C.c_void_p), n_masks=len(t_masks), out=t_out.data_ptr(), out_bytes=t_out.numel(),
             ws=t_ws.data_ptr(), ws_bytes=t_ws.numel())
    a.update(over)
    rc = _lib.lib().io_poly_fill_u8(C.c_void_p(a["verts"]), C.c_size_t(a["n_verts"]), C.c_void_p(a["parts_dev"]),
                                    a["parts_host"], a["n_parts"], C.c_void_p(a["masks_dev"]), a["masks_host"],
                                    a["n_masks"], C.c_void_p(a["out"]), C.c_size_t(a["out_bytes"]), C.c_void_p(a["ws"]),
                                    C.c_size_t(a["ws_bytes"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_fill_kernel_byte_exact_in_one_launch():
    """masks of different sizes in one launch; values 1 and 7; multi-part, zero-part, one- and two-vertex parts; polygons
    crossing and outside every side; whole images; the fixed vectors; planes of one, two and three scan passes; widths that
    are no multiple of 4; outputs at offsets of every alignment, odd ones included; guard bytes around every output"""
    cases = kernel_cases()
    assert any(len(c[0]) == 0 for c in cases) and any(len(c[0]) == 3 for c in cases)
    assert any(len(p) == 2 for c in cases for p in c[0]) and any(len(p) == 4 for c in cases for p in c[0])
    pms = [poly.PolyMasks([parts], H, W, values=[value]) for parts, H, W, value, _ in cases]
    offs, cursor = [], 0
    want_align = [16, 48, 16 + 64, 1, 2, 3, 32, 0, 5, 7]            # out_off mod 64, in turn
    for k, (parts, H, W, value, what) in enumerate(cases):
        cursor += GUARD
        cursor += (want_align[k % len(want_align)] - cursor) % 64
        offs.append(cursor)
        cursor += H * W
    total = cursor + GUARD
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    verts, parts_t, masks_t, n_parts = poly.descriptors([(pm, 0) for pm in pms], offs)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((poly.workspace_bytes(parts_t, n_parts, masks_t),), FILL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 64 == 0
    assert launch(verts, parts_t, n_parts, masks_t, out, ws) == 0, _lib.last_error()
    got = out.cpu().numpy()
    expect = np.full(total, FILL, np.uint8)
    nonempty = 0
    for (parts, H, W, value, what), o in zip(cases, offs):
        ref = oracle_mask(parts, H, W, value)
        assert np.array_equal(got[o:o + H * W].reshape(H, W), ref), what
        expect[o:o + H * W] = ref.reshape(-1)
        nonempty += int(ref.any())
        if what.startswith("the whole"):
            assert (ref == value).all(), what
    assert nonempty >= 30
    assert np.array_equal(got, expect), "a guard byte was written"
    # the same tables once more on the used workspace: the call clears its planes itself
    out.fill_(FILL)
    assert launch(verts, parts_t, n_parts, masks_t, out, ws) == 0, _lib.last_error()
    assert np.array_equal(out.cpu().numpy(), expect)


def test_decode_wrapper_and_profile_class():
    """poly.decode == to_dense() for polygons and run-length codes mixed in one image, into ``out`` too; the polygon call
    is timed under its own class"""
    H, W = 37, 29
    pool = random_instances(3, H, W, 30)
    inst = [pool[i] for i in (8, 9, 15, 17, 24, 4)] + [{"size": [H, W], "counts": [100, 200, H * W - 300]}]
    pm = poly.PolyMasks(inst, H, W, values=[1, 2, 3, 250, 255, 9, 77])
    L = _lib.lib()
    L.io_prof_begin_ex(0)
    got = poly.decode(pm, "cuda:0")
    ent = (_lib.ProfEntry * 32)()
    n = L.io_prof_end(ent, 32)
    dense = pm.to_dense()
    assert dense[6].max() == 77 and all(dense[i].any() for i in range(5)) and not dense[5].any()
    assert np.array_equal(got.cpu().numpy(), dense)
    assert [e.launches for e in ent[:n] if e.name == b"poly_fill"] == [1]
    assert [e.launches for e in ent[:n] if e.name == b"rle_decode"] == [1]
    out = torch.full((7, H, W), FILL, dtype=torch.uint8, device="cuda")
    assert pm.to_device("cuda:0", out=out) is out and np.array_equal(out.cpu().numpy(), dense)
    assert np.array_equal(pm[[6, 2]].to_device("cuda:0").cpu().numpy(), dense[[6, 2]])
    assert poly.decode(pm[[]], "cuda:0").shape == (0, H, W)
    with pytest.raises(ValueError):
        poly.decode(pm, "cuda:0", out=torch.empty((7, H, W + 1), dtype=torch.uint8, device="cuda"))


def test_entry_point_refusals():
    """every condition the entry point validates, on the HOST copy of the tables (the device copies stay valid): the error
    code, a message, no launch, and `out` with its guard bytes as it was"""
    H, W = 5, 3
    pm = poly.PolyMasks([[[0.5, 0.5, 2.5, 0.5, 2.5, 4.5], [0, 0, 1, 1]], [[1, 1, 2, 4, 0, 3]]], H, W)
    out = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    L = _lib.lib()

    def tables():
        return poly.descriptors([(pm, 0), (pm, 1)], [16, 48])

    verts, parts0, masks0, n_parts = tables()
    ws = torch.full((poly.workspace_bytes(parts0, n_parts, masks0) + 16,), FILL, dtype=torch.uint8, device="cuda")

    def call(mask=None, part=None, which=0, device_too=False, **over):
        verts, parts, masks, n_parts = tables()
        for k, v in (mask or {}).items():
            setattr(masks[which], k, v)
        for k, v in (part or {}).items():
            setattr(parts[which], k, v)
        if not device_too:
            over.update(parts_dev_table=parts0, masks_dev_table=masks0)
        return launch(verts, parts, n_parts, masks, out, ws, **over)

    L.io_prof_begin_ex(0)
    refused = [
        (call(mask=dict(H=0)), "size"), (call(mask=dict(W=-3)), "size"), (call(mask=dict(H=1 << 16, W=1 << 15)), "size"),
        (call(mask=dict(value=256)), "value"), (call(mask=dict(value=-1)), "value"),
        (call(mask=dict(first_part=-1)), "outside the part table"), (call(mask=dict(n_parts=4)), "outside the part table"),
        (call(mask=dict(n_parts=-1)), "outside the part table"),
        (call(mask=dict(n_parts=3)), "names mask"),            # mask 0 claims a part of mask 1
        (call(mask=dict(n_parts=1)), "own"),                   # part 1 is nobody's
        (call(part=dict(mask=1)), "names mask"), (call(part=dict(mask=-1)), "names mask"),
        (call(part=dict(n_verts=0)), "n_verts"),
        (call(part=dict(vert_off=-1)), "vertex buffer"), (call(part=dict(n_verts=4), which=2), "vertex buffer"),
        (call(n_verts=7), "vertex buffer"),                     # the last part ends one vertex past the buffer
        (call(mask=dict(out_off=-1)), "output"), (call(mask=dict(out_off=256 - 14), which=1), "output"),
        (call(out_bytes=62), "output"),
        (call(n_masks=0), "empty"), (call(n_masks=65536), "65535"), (call(n_parts=-1), "n_parts"),
        (call(ws=ws.data_ptr() + 4), "aligned"),
        (call(out=0), "null"), (call(ws=0), "null"), (call(masks_dev=0), "null"), (call(parts_dev=0), "null"),
        (call(verts=0), "null"), (call(masks_host=None), "null"), (call(parts_host=None), "null"),
    ]
    for k, (rc, _) in enumerate(refused):
        assert rc == -1, (k, rc)
    assert call(ws_bytes=ws.numel() - 17) == -2 and "workspace" in _lib.last_error()       # IO_ERR_WORKSPACE
    # the messages: each call again, reading the message straight after it
    assert call(mask=dict(value=256)) == -1 and "value" in _lib.last_error()
    assert call(part=dict(n_verts=4), which=2) == -1 and "vertex buffer" in _lib.last_error()
    assert call(mask=dict(out_off=256 - 14), which=1) == -1 and "output" in _lib.last_error()
    assert call(mask=dict(n_parts=1)) == -1 and "own" in _lib.last_error()
    assert call(n_masks=65536) == -1 and "65535" in _lib.last_error()
    assert call(ws=ws.data_ptr() + 4) == -1 and "aligned" in _lib.last_error()
    ent = (_lib.ProfEntry * 32)()
    assert L.io_prof_end(ent, 32) == 0, "a refused call launched something"
    assert bool((out == FILL).all()) and bool((ws == FILL).all())
    assert call(mask=dict(out_off=256 - 15), which=1, device_too=True, ws_bytes=ws.numel() - 16) == 0    # inside by one byte
    got = out.cpu().numpy()
    dense = pm.to_dense()
    assert np.array_equal(got[16:31].reshape(H, W), dense[0]) and np.array_equal(got[241:256].reshape(H, W), dense[1])
    assert (got[:16] == FILL).all() and (got[31:241] == FILL).all() and dense.any()


def test_renderer_poly_equals_dense_bit_for_bit():
    """polygon, run-length and dense images mixed in one batch (one polygon image holds a run-length instance, one is
    category-valued), with and without the image: the planes of the same call on dense masks; the upload counts the
    vertices, not H * W per mask"""
    S = 32
    rng = np.random.RandomState(11)
    sizes = [(61, 83), (120, 47), (33, 33)]
    images = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in sizes]
    pms = []
    for k, (H, W) in enumerate(sizes):
        rs = np.random.RandomState(20 + k)
        inst = [[random_part(rs, H, W, "cent", k=6)], [random_part(rs, H, W, "half", k=5), random_part(rs, H, W, "int", k=4)],
                [[-5.5, H / 2, W / 2, -4.25, W + 3, H * 0.8, W / 3, H + 6]]]          # crosses all four sides
        pms.append(poly.PolyMasks(inst, H, W))
    H1, W1 = sizes[1]
    rs = np.random.RandomState(29)                      # image 1: a crowd region among the polygons, and a category id
    pms[1] = poly.PolyMasks([[random_part(rs, H1, W1, "cent", k=6)], {"size": [H1, W1], "counts": [500, 700, H1 * W1 - 1200]},
                             [[-5.5, H1 / 2, W1 / 2, -4.25, W1 + 3, H1 * 0.8, W1 / 3, H1 + 6]]], H1, W1, values=[1, 1, 7])
    dense = [p.to_dense() for p in pms]
    assert all(d[i].any() for d in dense for i in range(3)) and dense[1][2].max() == 7
    items = []
    for ii, (H, W) in enumerate(sizes):
        boxes = [(0, 0, W, H), (-9, -13, W + 20, H + 30), (W // 3, H // 4, 11, 11), (W - 5, H - 6, 40, 40),
                 (2, 3, 3 * S, 3 * S), (1, 1, 1, 1)]
        for k, box in enumerate(boxes):
            items.append((ii, k % 3, (k + 1) % 3, box, 1 + (k + ii) % 3, bool(k % 2)))
    want = [t.cpu().numpy() for t in datasets.PairRenderer(S, MEAN, STD).render(images, dense, items)]
    r = datasets.PairRenderer(S, MEAN, STD)
    mixed = [pms[0], rle.RLEMasks.from_dense(dense[1] != 0).with_values([1, 1, 7]), dense[2]]
    for name, mm in (("poly", pms), ("mixed", mixed), ("poly+dense", [dense[0], pms[1], pms[2]])):
        got = r.render(images, mm, items)
        for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
            assert np.array_equal(g.cpu().numpy(), w), (name, plane)
    r.render(images, pms, items)
    up = r.last_upload
    nverts = sum(V.shape[0] for p in pms for i in range(3) if p.is_polygon(i) for V in p.parts(i))
    run_entries = pms[1].rle_ref(1)[0].ends()[0].size
    assert up["images"] == sum(im.size for im in images)
    assert up["masks"] == 8 * nverts + 4 * run_entries
    assert up["masks"] < sum(d[0].size for d in dense) // 10
    assert up["total"] < up["images"] + up["masks"] + up["descriptors"] + 16 * 16
    rgb0, m1b, m2b = r.render(images, pms, items[:5], load_rgb=False)
    assert float(rgb0.abs().max()) == 0.0 and r.last_upload["images"] == 0
    assert np.array_equal(m1b.cpu().numpy(), want[1][:5]) and np.array_equal(m2b.cpu().numpy(), want[2][:5])
    rgb2, m1c, _ = r.render(images, pms, items[7:15])                    # both staging buffers have been used by now
    assert np.array_equal(rgb2.cpu().numpy(), want[0][7:15]) and np.array_equal(m1c.cpu().numpy(), want[1][7:15])


class _PolyReader(object):
    """a SyntheticReader whose instance masks are polygons (``dense``: the same masks rasterised)"""

    def __init__(self, reader, dense):
        self._reader, self._dense, self._cache = reader, dense, {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._reader, name)

    def get_image_instances(self, idx, *args, **kw):
        out = self._reader.get_image_instances(idx, *args, **kw)
        key = int(idx)
        if key not in self._cache:
            n, H, W = out[0].shape
            rs = np.random.RandomState(1000 + key)
            inst = []
            for i in range(n):
                x, y, w, h = [float(v) for v in out[2][i]]
                t = np.sort(rs.uniform(0, 2 * np.pi, 7))
                ring = np.stack([x + w / 2 + 0.6 * w * np.cos(t), y + h / 2 + 0.6 * h * np.sin(t)], axis=1)
                inst.append([np.round(ring, 2).reshape(-1).tolist()])
            pm = poly.PolyMasks(inst, H, W)
            self._cache[key] = (pm, pm.to_dense())
        return (self._cache[key][1 if self._dense else 0],) + tuple(out[1:])


@pytest.mark.parametrize("use_category", [False, True])
def test_batches_over_a_polygon_reader_equal_the_dense_reader(use_category):
    """SupOcclusionOrderBatches.batch() over polygon masks == over the same masks rasterised, with and without category
    values; ids above 255 are refused as for dense masks"""
    z = load_golden("dataset_items")
    cfg = dict(json.loads(str(z["config_json"])), patch_or_image="patch", use_category=use_category)
    outs = []
    for dense in (True, False):
        rd = _PolyReader(synthetic.SyntheticReader(int(z["reader_seed"])), dense)
        ds = datasets.SupOcclusionOrderBatches(cfg, "train", "InstaOrderNet_o", rd, rd.load_image)
        np.random.seed(101)
        outs.append(ds.batch(range(6)))
    assert len(outs[0]) == 4 and float(outs[0][1].abs().max()) > 0
    if use_category:
        assert float(outs[0][1].max()) > 1
    for f, (w, g) in enumerate(zip(*outs)):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w.cpu().numpy()), f
    if use_category:
        class Big(_PolyReader):
            def get_image_instances(self, idx, *args, **kw):
                out = _PolyReader.get_image_instances(self, idx, *args, **kw)
                return (out[0], np.asarray(out[1]) + 300) + tuple(out[2:])
        rd = Big(synthetic.SyntheticReader(int(z["reader_seed"])), False)
        ds = datasets.SupOcclusionOrderBatches(cfg, "train", "InstaOrderNet_o", rd, rd.load_image)
        with pytest.raises(ValueError, match="255"):
            ds.batch(range(2))


@pytest.fixture(scope="module")
def scene():
    rd = _PolyReader(synthetic.SyntheticReader(3), False)
    pm = rd.get_image_instances(0, with_gt=True)[0]
    return pm, pm.to_dense()


def test_mask_rules_pair_relations_and_select_pairs(scene):
    pm, dense = scene
    want, got = mask_rules.pair_relations(dense), mask_rules.pair_relations(pm)
    assert sorted(want) == sorted(got)
    for key in want:
        assert np.array_equal(want[key], got[key]), key
    assert want["area"].all() and (want["touch"] & ~np.eye(len(pm), dtype=bool)).any()
    want = mask_rules.pair_relations(dense, dense)["inter"]
    assert np.array_equal(want, mask_rules.pair_relations(pm, pm)["inter"]) and (want - np.diag(np.diag(want))).any()
    assert np.array_equal(mask_rules.infer_occ_order_area(dense), mask_rules.infer_occ_order_area(pm))
    want = mask_rules.select_pairs(dense, "nbor")
    assert want == inference.select_pairs(dense, "nbor") and len(want) > 0
    assert mask_rules.select_pairs(pm, "nbor") == want


@pytest.fixture(scope="module")
def net():
    import instaorder_amd as ia
    params = dict(algo="InstaOrderNet_o", lr=1e-3, weight_decay=1e-4, optim="SGD", use_rgb=True,
                  backbone_arch="resnet50_cls", backbone_param=dict(in_channels=5, num_classes=2))
    m = ia.InstaOrderNet_o(params, dist_model=False)
    m.switch_to("eval")
    return m


@pytest.mark.parametrize("mode", ["patch", "resize"])
def test_infer_order_sup_occ_poly_equals_dense(net, mode):
    """the same order matrix from polygon masks as from their dense form, with the device rules (the masks never exist on
    the host) and with the host rules (rasterised once)"""
    rd = synthetic.SyntheticReader(9, n_images=4, n_inst=4, empty_every=0)
    sc = rd.scenes[1]
    pm = _PolyReader(rd, False).get_image_instances(1, with_gt=True)[0]
    dense = pm.to_dense()
    want = inference.infer_order_sup_occ(net, sc["image"], dense, sc["bboxes"], "nbor", "InstaOrderNet_o", mode, 64)
    for rules in ("device", "host"):
        got = inference.infer_order_sup_occ(net, sc["image"], pm, sc["bboxes"], "nbor", "InstaOrderNet_o", mode, 64,
                                            mask_rules=rules)
        assert np.array_equal(got, want), rules
    assert want.shape == (4, 4)


def test_evaluate_over_a_polygon_reader_equals_the_dense_reader():
    """evaluate() with the model-free 'area' rule, category-valued masks, device and host rules"""
    from instaorder_amd import evaluate
    base = synthetic.SyntheticReader(5, n_images=3, n_inst=6, empty_every=0)
    cfg = dict(trainval_dataset="SupOcclusionOrderDataset", patch_or_image="patch", input_size=64, dataset="InstaOrder",
               enlarge_box=3.0, use_category=True, remove_occ_bidirec=0)
    rd = _PolyReader(base, True)
    want = evaluate.evaluate(None, rd, rd.load_image, cfg, "area", return_orders=True)
    for rules in ("device", "host"):
        rp = _PolyReader(base, False)
        got = evaluate.evaluate(None, rp, rp.load_image, cfg, "area", return_orders=True, mask_rules=rules)
        for key in ("recall", "precision", "f1"):
            assert want[key] == got[key], (rules, key)
        for i in range(3):
            assert np.array_equal(want["orders"][i][0], got["orders"][i][0]), (rules, i)
