"""Baseline JPEG files on the MI355X: io_jpeg_decode_u8 (csrc/jpeg.hip) byte for byte against what the reference's
``Image.open(f).convert('RGB')`` made of the fixture files (tests/golden/jpeg_cases.npz), its refusals, damaged streams, and
every consumer of ``jpeg.JpegImage`` against the same call on the decoded arrays: the renderer, the dataset classes, the
inference driver and evaluate()."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import jpeg_cases
from helpers import load_golden
from instaorder_amd import _lib, datasets, inference, jpeg, poly, rle, synthetic

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
GUARD, FILL = 48, 0xAB
NAMES, CASES, _ = jpeg_cases.load()


def upload(a):
    a = np.frombuffer(a, dtype=np.uint8) if not isinstance(a, np.ndarray) else a
    return torch.from_numpy(a.copy() if a.size else np.zeros(16, np.uint8)).cuda()


def launch(t_pool, t_tables, t_desc, t_out, t_ws, t_status, **over):
    """io_jpeg_decode_u8 with device copies of the tables as given; ``over`` replaces single arguments of the call"""
    keep = [upload(t_pool), upload(over.pop("tables_dev_table", t_tables)), upload(over.pop("desc_dev_table", t_desc))]
    a = dict(pool=keep[0].data_ptr(), pool_bytes=t_pool.size, tables_dev=keep[1].data_ptr(),
             tables_host=t_tables.ctypes.data_as(C.c_void_p), tables_bytes=t_tables.size, desc_dev=keep[2].data_ptr(),
             desc_host=C.cast(t_desc, C.c_void_p), n=len(t_desc), out=t_out.data_ptr(), out_bytes=t_out.numel(),
             ws=t_ws.data_ptr(), ws_bytes=t_ws.numel(), status=t_status.data_ptr())
    a.update(over)
    rc = _lib.lib().io_jpeg_decode_u8(C.c_void_p(a["pool"]), C.c_size_t(a["pool_bytes"]), C.c_void_p(a["tables_dev"]),
                                      a["tables_host"], C.c_size_t(a["tables_bytes"]), C.c_void_p(a["desc_dev"]),
                                      a["desc_host"], a["n"], C.c_void_p(a["out"]), C.c_size_t(a["out_bytes"]),
                                      C.c_void_p(a["ws"]), C.c_size_t(a["ws_bytes"]), C.c_void_p(a["status"]),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def offsets(images):
    """output offsets of every alignment, odd ones included, with guard bytes between the images"""
    offs, cursor = [], 0
    want_align = [16, 48, 16 + 64, 1, 2, 3, 32, 0, 5, 7]
    for k, im in enumerate(images):
        cursor += GUARD
        cursor += (want_align[k % len(want_align)] - cursor) % 64
        offs.append(cursor)
        cursor += im.H * im.W * 3
    return offs, cursor + GUARD


def test_decode_kernels_byte_exact_in_one_call():
    """every fixture case -- 1x1 to 160x208, 4:4:4 / 4:2:2 / 4:2:0 / grayscale, qualities 30 to 100, optimised tables,
    restart intervals -- in ONE call; outputs at offsets of every alignment with guard bytes around them; all status words
    zero; the same once more on the used workspace (the call clears its coefficients itself)"""
    ims = [jpeg_cases.image(n) for n in NAMES]
    offs, total = offsets(ims)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    pool, tables, desc = jpeg.descriptors(ims, offs)
    assert tables.size // jpeg.TABLES_BYTES < len(ims) // 2          # shared table sets are uploaded once
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((jpeg.workspace_bytes(desc),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 64 == 0
    assert launch(pool, tables, desc, out, ws, status) == 0, _lib.last_error()
    assert status.cpu().numpy().tolist() == [0] * len(ims)
    got = out.cpu().numpy()
    expect = np.full(total, FILL, np.uint8)
    for name, im, o in zip(NAMES, ims, offs):
        ref = CASES[name][1]
        g = got[o:o + ref.size].reshape(ref.shape)
        assert np.array_equal(g, ref), "%s: %d of %d bytes differ" % (name, (g != ref).sum(), ref.size)
        expect[o:o + ref.size] = ref.reshape(-1)
    assert np.array_equal(got, expect), "a guard byte was written"
    out.fill_(FILL)
    status.fill_(-1)
    lanes = _lib.lib().io_jpeg_get_images_per_wave()
    try:                                                    # a full wave of images, then five per wave: the same bytes
        assert _lib.lib().io_jpeg_set_images_per_wave(64) == 0
        assert launch(pool, tables, desc, out, ws, status) == 0, _lib.last_error()
        assert np.array_equal(out.cpu().numpy(), expect) and not status.cpu().numpy().any()
        out.fill_(FILL)
        status.fill_(-1)
        assert _lib.lib().io_jpeg_set_images_per_wave(5) == 0
        assert launch(pool, tables, desc, out, ws, status) == 0, _lib.last_error()
    finally:
        _lib.lib().io_jpeg_set_images_per_wave(lanes)
    assert np.array_equal(out.cpu().numpy(), expect) and not status.cpu().numpy().any()
    # that call had more table sets than fit in LDS (the tables were read from global memory); now every case once more
    # in calls of at most io_jpeg_lds_table_sets() sets each, which decode with their tables in LDS
    cap = _lib.lib().io_jpeg_lds_table_sets()
    assert tables.size // jpeg.TABLES_BYTES > cap
    groups, sets = [[]], set()
    for k, im in enumerate(ims):
        if len(sets | {im.tables_blob()}) > cap:
            groups.append([])
            sets = set()
        sets.add(im.tables_blob())
        groups[-1].append(k)
    out.fill_(FILL)
    for g in groups:
        pool_g, tables_g, desc_g = jpeg.descriptors([ims[k] for k in g], [offs[k] for k in g])
        assert tables_g.size // jpeg.TABLES_BYTES <= cap
        st_g = torch.full((len(g),), -1, dtype=torch.int32, device="cuda")
        assert launch(pool_g, tables_g, desc_g, out, ws, st_g) == 0, _lib.last_error()
        assert not st_g.cpu().numpy().any()
    assert len(groups) >= 2 and np.array_equal(out.cpu().numpy(), expect)


def test_decode_list_and_out():
    names = ["33x47_420_q85", "1x1_gray_q85", "21x35_422_rst2"]
    ims = [jpeg_cases.image(n) for n in names]
    got = jpeg.decode(ims, "cuda")
    for g, n in zip(got, names):
        assert g.is_cuda and g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), CASES[n][1]), n
    out = torch.zeros(3 * (33 * 47 + 1 + 21 * 35) + 64, dtype=torch.uint8, device="cuda")
    got = jpeg.decode(ims, "cuda", out=out)
    assert got[0].data_ptr() == out.data_ptr() and np.array_equal(got[2].cpu().numpy(), CASES[names[2]][1])
    with pytest.raises(ValueError, match="out must be"):
        jpeg.decode(ims, "cuda", out=out[:100])
    with pytest.raises(ValueError, match="not supported"):
        jpeg.decode([jpeg.JpegImage(jpeg_cases.load()[2]["progressive"])], "cuda")
    assert jpeg.decode([], "cuda") == []


def test_entry_point_refusals_launch_nothing():
    ims = [jpeg_cases.image(n) for n in ("9x17_420_q85", "21x35_444_rst2")]
    sizes = [im.H * im.W * 3 for im in ims]
    pool, tables, desc0 = jpeg.descriptors(ims, [16, 1024])
    out = torch.full((1024 + sizes[1],), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((jpeg.workspace_bytes(desc0),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call(d=None, which=0, table=None, **over):
        desc = (_lib.JpegDesc * 2)()
        C.memmove(desc, desc0, C.sizeof(desc0))
        for k, v in (d or {}).items():
            if isinstance(v, tuple):
                getattr(desc[which], k)[v[0]] = v[1]
            else:
                setattr(desc[which], k, v)
        tabs = tables.copy()
        if table is not None:
            tabs[table[0]] = table[1]
        return launch(pool, tabs, desc, out, ws, status, desc_dev_table=desc0, tables_dev_table=tables, **over)

    L.io_prof_begin_ex(0)
    ac0_counts = 512 + 2 * 16                                   # the code-length counts of AC table 0
    refused = [
        (call(dict(hs=1, vs=2)), "sampling"), (call(dict(hs=4)), "sampling"), (call(dict(n_comp=4)), "components"),
        (call(dict(n_comp=1)), "components"),                   # one component with 2 x 2 sampling
        (call(dict(H=0)), "size"), (call(dict(W=65536)), "size"), (call(dict(restart_interval=-1)), "restart_interval"),
        (call(dict(table_set=1)), "table set"), (call(dict(table_set=-1)), "table set"),
        (call(dict(quant=(1, 4))), "quant"), (call(dict(dc=(0, 2))), "Huffman"), (call(dict(ac=(2, 3)), which=1), "Huffman"),
        (call(table=(ac0_counts, 3)), "prefix code"),           # three codes of one bit: over-subscribed
        (call(table=(ac0_counts + 15, 255)), "prefix code"),    # more than 256 symbols
        (call(dict(data_off=-1)), "data range"), (call(dict(data_bytes=-5)), "data range"),
        (call(dict(data_bytes=desc0[1].data_bytes + 1), which=1), "byte pool"), (call(pool_bytes=pool.size - 1), "byte pool"),
        (call(dict(out_off=-1)), "output"), (call(dict(out_off=1024 + 1), which=1), "output"),
        (call(out_bytes=1024 + sizes[1] - 1), "output"),
        (call(tables_bytes=jpeg.TABLES_BYTES - 1), "table set"),
        (call(n=0), "empty"), (call(n=65536), "65535"),
        (call(ws=ws.data_ptr() + 4), "aligned"),
        (call(out=0), "null"), (call(ws=0), "null"), (call(pool=0), "null"), (call(status=0), "null"),
        (call(tables_dev=0), "null"), (call(tables_host=None), "null"), (call(desc_dev=0), "null"),
    ]
    for k, (rc, _) in enumerate(refused):
        assert rc == -1, (k, rc)
    assert call(desc_host=None) == -1
    assert call(ws_bytes=ws.numel() - 1) == -2 and "workspace" in _lib.last_error()        # IO_ERR_WORKSPACE
    assert call(dict(hs=1, vs=2)) == -1 and "sampling" in _lib.last_error()
    assert call(dict(dc=(0, 2))) == -1 and "Huffman < 2" in _lib.last_error()
    assert call(table=(ac0_counts, 3)) == -1 and "prefix code" in _lib.last_error()
    assert call(dict(data_bytes=desc0[1].data_bytes + 1), which=1) == -1 and "byte pool" in _lib.last_error()
    assert call(out_bytes=1024 + sizes[1] - 1) == -1 and "output" in _lib.last_error()
    ent = (_lib.ProfEntry * 32)()
    assert L.io_prof_end(ent, 32) == 0, "a refused call launched something"
    assert bool((out == FILL).all()) and bool((ws == FILL).all()) and bool((status == -1).all())
    assert call() == 0, _lib.last_error()                       # and the tables as they are decode
    got = out.cpu().numpy()
    for (o, n), name in zip(((16, sizes[0]), (1024, sizes[1])), ("9x17_420_q85", "21x35_444_rst2")):
        assert np.array_equal(got[o:o + n], CASES[name][1].reshape(-1))
    assert (got[:16] == FILL).all() and (got[16 + sizes[0]:1024] == FILL).all()


def test_damaged_streams_are_flagged_and_leave_their_neighbours_alone():
    """truncations and mutations that tests/jpeg_entropy_host.cpp ran under the sanitizers (tests/test_jpeg_cpu.py), between
    intact images in one call: the status word is what ``JpegImage.coefficients`` says -- non-zero for exactly the streams
    that do not decode -- the neighbours are byte exact, guard bytes stay, and jpeg.decode raises naming the image"""
    ims, want, pixels = [], [], []
    for s, name in enumerate(jpeg_cases.FUZZ):
        base = jpeg_cases.image(name)
        ent = base.entropy_bytes()
        alts = [base.with_entropy(ent[:len(ent) // 3], name + " cut at a third"), base.with_entropy(ent[:-1], name + " cut by one"),
                base.with_entropy(b"", name + " empty")]
        alts += [base.with_entropy(jpeg_cases.mutated(ent, m), "%s mutation %d" % (name, m)) for m in range(4 * s, 4 * s + 4)]
        for alt in alts:
            ims += [base, alt]
            st = jpeg_cases.status_of(alt)[0]
            want += [0, st]
            pixels += [CASES[name][1], alt.to_host() if st == 0 else None]
    assert sum(1 for w in want if w) >= 9 and len(set(want)) >= 3
    offs, total = offsets(ims)
    pool, tables, desc = jpeg.descriptors(ims, offs)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.empty(jpeg.workspace_bytes(desc), dtype=torch.uint8, device="cuda")
    status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    assert launch(pool, tables, desc, out, ws, status) == 0, _lib.last_error()
    assert status.cpu().numpy().tolist() == want
    got = out.cpu().numpy()
    covered = np.zeros(total, bool)
    for im, o, ref in zip(ims, offs, pixels):
        n = im.H * im.W * 3
        covered[o:o + n] = True
        if ref is not None:
            assert np.array_equal(got[o:o + n].reshape(ref.shape), ref), im.name
    assert (got[~covered] == FILL).all(), "a guard byte was written"
    bad = next(im for im, w in zip(ims, want) if w)
    with pytest.raises(RuntimeError, match="cut at a third"):
        jpeg.decode([ims[0], bad, ims[0]], "cuda")


def _mixed_batch():
    """three images: two JPEG files and one array; run-length, polygon and dense masks"""
    names = ["33x47_420_q85", "40x24_422_q85", "21x35_444_q85"]
    arrays = [CASES[n][1] for n in names]
    jp = [jpeg_cases.image(names[0]), jpeg_cases.image(names[1]), arrays[2]]
    masks = []
    for k, a in enumerate(arrays):
        H, W = a.shape[:2]
        y, x = np.mgrid[0:H, 0:W]
        m = np.stack([(x > W // 4) & (y < 2 * H // 3), (x - W / 2) ** 2 + (y - H / 2) ** 2 < (min(H, W) / 3) ** 2,
                      (x + y) % 7 < 3]).astype(np.uint8)
        masks.append(m)
    H1, W1 = arrays[1].shape[:2]
    pm = poly.PolyMasks([[[2.5, 3.0, W1 - 3.0, 4.5, W1 / 2, H1 - 2.0]], [[-4, -3, W1 + 2, H1 / 2, 3, H1 + 5]],
                         [[1, 1, W1 - 1, 1, W1 - 1, H1 - 1, 1, H1 - 1]]], H1, W1)
    masks[1] = pm.to_dense()
    enc = [rle.RLEMasks.from_dense(masks[0] != 0), pm, masks[2]]
    items = []
    for ii, a in enumerate(arrays):
        H, W = a.shape[:2]
        hw = max(H, W)
        boxes = [((W // 4 - 6, H // 4 - 5, 27, 27), datasets.INTER_CUBIC),                # 'patch'
                 ((0, 0, W, H), datasets.INTER_LINEAR),                                    # 'resize'
                 ((-((hw - W) // 2), -((hw - H) // 2), hw, hw), datasets.INTER_LINEAR)]    # 'image'
        for k, (box, interp) in enumerate(boxes):
            items.append((ii, k % 3, (k + 1) % 3, box, interp, bool((k + ii) % 2)))
    return arrays, jp, masks, enc, items[:8]


def test_renderer_jpeg_equals_arrays_bit_for_bit():
    S = 64
    arrays, jp, masks, enc, items = _mixed_batch()
    assert len(items) == 8 and {it[0] for it in items} == {0, 1, 2} and any(it[5] for it in items)
    want = [t.cpu().numpy() for t in datasets.PairRenderer(S, MEAN, STD).render(arrays, masks, items)]
    assert np.abs(want[0]).max() > 0 and want[1].any()
    r = datasets.PairRenderer(S, MEAN, STD)
    for name, ii, mm in (("jpeg + dense masks", jp, masks), ("jpeg + encoded masks", jp, enc), ("arrays + encoded", arrays, enc),
                         ("all jpeg", [jp[0], jp[1], jpeg_cases.image("21x35_444_q85")], enc)):
        got = r.render(ii, mm, items)
        for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
            assert np.array_equal(g.cpu().numpy(), w), (name, plane)
    r.render(jp, enc, items)
    up = r.last_upload
    tables = len({jp[0].tables_blob(), jp[1].tables_blob()}) * jpeg.TABLES_BYTES
    assert up["images"] == arrays[2].size + jp[0].nbytes_entropy + jp[1].nbytes_entropy + tables
    assert up["images"] < sum(a.size for a in arrays)
    r.render(jp[:2] + [None], enc, [it for it in items if it[0] < 2])
    assert r.last_upload["images"] == jp[0].nbytes_entropy + jp[1].nbytes_entropy + tables        # the compressed bytes
    rgb0, m1, m2 = r.render(jp, enc, items, load_rgb=False)
    assert float(rgb0.abs().max()) == 0.0 and r.last_upload["images"] == 0
    assert np.array_equal(m1.cpu().numpy(), want[1]) and np.array_equal(m2.cpu().numpy(), want[2])
    r.check_status()
    # a stream that does not decode is reported when its staging slot comes round again, or by check_status()
    broken = jp[0].with_entropy(jp[0].entropy_bytes()[:40], "broken.jpg")
    r.render([broken, jp[1], arrays[2]], enc, items)
    with pytest.raises(RuntimeError, match="broken.jpg"):
        r.check_status()
    r.render([broken, jp[1], arrays[2]], enc, items)
    r.render(jp, enc, items)
    with pytest.raises(RuntimeError, match="broken.jpg"):
        r.render(jp, enc, items)
    r.check_status()


class _JpegReader(object):
    """a SyntheticReader whose scenes all show the 160 x 208 fixture image: the masks are padded to that size, and
    ``load_image`` returns the file as a ``JpegImage`` or (``as_jpeg`` False) the array the reference's load gives"""
    NAME = "160x208_420_q90"

    def __init__(self, reader, as_jpeg):
        self._reader, self._as_jpeg, self._cache = reader, as_jpeg, {}
        self.loads = 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._reader, name)

    @staticmethod
    def _pad(m):
        if m is None:
            return None
        out = np.zeros((m.shape[0], 160, 208), m.dtype)
        out[:, :m.shape[1], :m.shape[2]] = m
        return out

    def get_image_instances(self, idx, *args, **kw):
        key = int(idx)
        if key not in self._cache:
            out = self._reader.get_image_instances(idx, *args, **kw)
            self._cache[key] = (self._pad(out[0]), out[1], out[2], self._pad(out[3]), out[4])
        return self._cache[key]

    def load_image(self, image_fn):
        self.loads += 1
        return jpeg_cases.image(self.NAME) if self._as_jpeg else CASES[self.NAME][1]


@pytest.mark.parametrize("cls,algo", [(datasets.SupOcclusionOrderBatches, "InstaOrderNet_o"),
                                      (datasets.SupDepthOccOrderBatches, "InstaOrderNet_od")])
def test_batches_over_a_jpeg_reader_equal_the_array_reader(cls, algo):
    z = load_golden("dataset_items")
    cfg = dict(json.loads(str(z["config_json"])), patch_or_image="patch")
    outs = []
    for as_jpeg in (False, True):
        rd = _JpegReader(synthetic.SyntheticReader(int(z["reader_seed"])), as_jpeg)
        ds = cls(cfg, "train", algo, rd, rd.load_image, rng=np.random.RandomState(101))
        outs.append(ds.batch(range(6)))
        ds.renderer.check_status()
    assert float(outs[0][0].abs().max()) > 0 and float(outs[0][1].abs().max()) > 0
    for f, (w, g) in enumerate(zip(*outs)):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w.cpu().numpy()), f
    assert ds.renderer.last_upload["images"] <= 6 * len(CASES[_JpegReader.NAME][0]) < 6 * CASES[_JpegReader.NAME][1].size // 3


def test_prefetcher_reports_a_broken_file_at_its_end():
    z = load_golden("dataset_items")
    cfg = dict(json.loads(str(z["config_json"])), patch_or_image="patch")
    rd = _JpegReader(synthetic.SyntheticReader(int(z["reader_seed"])), True)
    good = jpeg_cases.image(_JpegReader.NAME)
    rd.load_image = lambda fn: good.with_entropy(good.entropy_bytes()[:100], "half.jpg")
    ds = datasets.SupOcclusionOrderBatches(cfg, "train", "InstaOrderNet_o", rd, rd.load_image, rng=np.random.RandomState(5))
    pf = datasets.BatchPrefetcher(ds, [[0, 1], [2, 3]])
    with pytest.raises(RuntimeError, match="half.jpg"):
        for _ in pf:
            pass


@pytest.fixture(scope="module")
def net():
    import instaorder_amd as ia
    params = dict(algo="InstaOrderNet_o", lr=1e-3, weight_decay=1e-4, optim="SGD", use_rgb=True,
                  backbone_arch="resnet50_cls", backbone_param=dict(in_channels=5, num_classes=2))
    m = ia.InstaOrderNet_o(params, dist_model=False)
    m.switch_to("eval")
    return m


@pytest.mark.parametrize("mode", ["patch", "resize"])
def test_infer_order_sup_occ_jpeg_equals_array(net, mode):
    rd = _JpegReader(synthetic.SyntheticReader(9, n_images=4, n_inst=4, empty_every=0), True)
    modal, _, bboxes, _, _ = rd.get_image_instances(1, with_gt=True)
    want = inference.infer_order_sup_occ(net, CASES[rd.NAME][1], modal, bboxes, "nbor", "InstaOrderNet_o", mode, 64)
    got = inference.infer_order_sup_occ(net, jpeg_cases.image(rd.NAME), modal, bboxes, "nbor", "InstaOrderNet_o", mode, 64)
    assert want.shape == (4, 4) and np.array_equal(got, want)
    im = jpeg_cases.image(rd.NAME)
    with pytest.raises(RuntimeError, match="cut.jpg"):
        inference.infer_order_sup_occ(net, im.with_entropy(im.entropy_bytes()[:64], "cut.jpg"), modal, bboxes, "nbor",
                                      "InstaOrderNet_o", mode, 64)


def test_evaluate_over_a_jpeg_reader_equals_the_array_reader(net):
    from instaorder_amd import evaluate
    base = synthetic.SyntheticReader(5, n_images=3, n_inst=4, empty_every=0)
    cfg = dict(trainval_dataset="SupOcclusionOrderDataset", patch_or_image="patch", input_size=64, dataset="InstaOrder",
               enlarge_box=3.0, use_category=False, remove_occ_bidirec=0)
    res = []
    for as_jpeg in (False, True):
        rd = _JpegReader(base, as_jpeg)
        res.append(evaluate.evaluate(net, rd, rd.load_image, cfg, "InstaOrderNet_o", return_orders=True))
        assert rd.loads == 3
    want, got = res
    for key in ("recall", "precision", "f1"):
        assert want[key] == got[key], key
    for i in range(3):
        assert np.array_equal(want["orders"][i][0], got["orders"][i][0]), i
