"""PNG files on the MI355X: io_png_decode (csrc/png.hip, csrc/png_inflate.h) byte for byte against ``PngImage.to_host()``
on a mixed batch built so that every size edge, form, filter type and DEFLATE stream property occurs (tests/png_cases.py),
damaged streams, the entry point's refusals, and the consumers of ``png.PngImage`` against the same call on the decoded
arrays: the renderer, a dataset class, the prefetcher and the dense KITTI evaluation."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import jpeg_cases
import png_cases
from helpers import load_golden
from instaorder_amd import _lib, datasets, png, synthetic
from test_gpu_jpeg import _JpegReader, _mixed_batch

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
GUARD, FILL = 48, 0xAB


def upload(a):
    a = np.frombuffer(a, dtype=np.uint8) if not isinstance(a, np.ndarray) else a
    return torch.from_numpy(a.copy() if a.size else np.zeros(16, np.uint8)).cuda()


def launch(t_pool, t_desc, t_out, t_ws, t_status, **over):
    """io_png_decode with device copies of the tables as given; ``over`` replaces single arguments of the call"""
    keep = [upload(t_pool), upload(over.pop("desc_dev_table", t_desc))]
    a = dict(pool=keep[0].data_ptr(), pool_bytes=t_pool.size, desc_dev=keep[1].data_ptr(), desc_host=C.cast(t_desc, C.c_void_p),
             n=len(t_desc), out=t_out.data_ptr(), out_bytes=t_out.numel(), ws=t_ws.data_ptr(), ws_bytes=t_ws.numel(),
             status=t_status.data_ptr())
    a.update(over)
    rc = _lib.lib().io_png_decode(C.c_void_p(a["pool"]), C.c_size_t(a["pool_bytes"]), C.c_void_p(a["desc_dev"]), a["desc_host"],
                                  a["n"], C.c_void_p(a["out"]), C.c_size_t(a["out_bytes"]), C.c_void_p(a["ws"]),
                                  C.c_size_t(a["ws_bytes"]), C.c_void_p(a["status"]),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def offsets(images):
    """output offsets of every alignment, odd ones included (even ones for the 16-bit form), with guard bytes between"""
    offs, cursor = [], 0
    want_align = [16, 49, 16 + 64, 1, 2, 3, 32, 0, 5, 7]
    for k, im in enumerate(images):
        cursor += GUARD
        cursor += (want_align[k % len(want_align)] - cursor) % 64
        if im.raw16 and cursor % 2:
            cursor += 1
        offs.append(cursor)
        cursor += im.out_bytes
    return offs, cursor + GUARD


def run(ims):
    offs, total = offsets(ims)
    pool, desc = png.descriptors(ims, offs)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((png.workspace_bytes(desc),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 64 == 0
    assert launch(pool, desc, out, ws, status) == 0, _lib.last_error()
    return offs, total, out.cpu().numpy(), status.cpu().numpy().tolist()


def test_decode_kernels_byte_exact_in_one_call():
    """ONE call over: sizes 1x1, 1xW, Hx1, W = 5; heights on both sides of the unfilter band; all four forms with every
    filter type forced on every row and a seeded mix; one image per stream property (asserted present first); IDAT in
    1-byte chunks.  Outputs at offsets of every alignment with guard bytes around them; all status words zero."""
    assert _lib.lib().io_png_band_rows() == png.UNFILTER_BAND
    cases = png_cases.batch_cases()
    for im, want, check in png_cases.stream_cases():
        st = im.stream_stats()
        assert check(st), "%s lost its property: %s" % (im.name, st)
        cases.append((im, want))
    ims = [c[0] for c in cases]
    assert {(im.H, im.W) for im in ims} >= {(1, 1), (1, 37), (41, 1), (7, 5)}
    assert {im.H for im in ims} >= {png.UNFILTER_BAND + d for d in (-1, 0, 1)} | {2 * png.UNFILTER_BAND + 1}
    assert {(im.channels, im.bit_depth) for im in ims} == {(3, 8), (4, 8), (1, 8), (1, 16)}
    assert max(len(im.chunks) for im in ims) > 100
    offs, total, got, status = run(ims)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    assert status == [0] * len(ims)
    expect = np.full(total, FILL, np.uint8)
    for (im, want), o in zip(cases, offs):
        ref = im.to_host()
        assert ref.dtype == want.dtype and np.array_equal(ref, want), im.name
        ref = ref.reshape(-1).view(np.uint8)
        g = got[o:o + ref.size]
        assert np.array_equal(g, ref), "%s: %d of %d bytes differ" % (im.name, (g != ref).sum(), ref.size)
        expect[o:o + ref.size] = ref
    assert np.array_equal(got, expect), "a guard byte was written"


def test_fixture_files_and_decode_list():
    names, CASES, unsupported = png_cases.load()
    ims = [png.PngImage(CASES[n][0], name=n) for n in names]
    got = png.decode(ims, "cuda")
    for g, n in zip(got, names):
        ref = CASES[n][1]
        assert g.is_cuda and g.dtype == (torch.uint16 if ref.dtype == np.uint16 else torch.uint8), n
        assert g.shape == ref.shape and np.array_equal(g.cpu().numpy(), ref), n
    d16 = next(g for g in got if g.dtype == torch.uint16)
    assert d16.view(torch.int16).shape == d16.shape                  # the storage depth_errors_median takes
    out = torch.zeros(sum((im.out_bytes + 15) // 16 * 16 for im in ims), dtype=torch.uint8, device="cuda")
    again = png.decode(ims, "cuda", out=out)
    assert again[0].data_ptr() == out.data_ptr() and np.array_equal(again[-1].cpu().numpy(), CASES[names[-1]][1])
    with pytest.raises(ValueError, match="out must be"):
        png.decode(ims, "cuda", out=out[:100])
    with pytest.raises(ValueError, match="not supported"):
        png.decode([png.PngImage(unsupported["palette"])], "cuda")
    assert png.decode([], "cuda") == []


def test_damaged_streams_are_flagged_and_leave_their_neighbours_alone():
    """the streams tests/png_inflate_host.cpp ran under the sanitizers (tests/test_png_cpu.py), every one behind an intact
    image in one call: status 0 exactly where ``to_host()`` succeeds, with equal bytes there; the documented word for each
    hand-made stream; the neighbours byte exact; guard bytes intact; png.decode raises naming the image"""
    good = png_cases.per_status()[0]
    ims, want, pixels = [], [], []
    for label, im in png_cases.damaged():
        try:
            px, st = im.to_host(), 0
        except png.PngStreamError as e:
            px, st = None, e.status
        ims += [good, im]
        want += [0, st]
        pixels += [good.to_host(), px]
    hand = {im.name: s for s, im in png_cases.per_status().items() if s}
    hand.update({im.name: s for im, s in png_cases.more_statuses()})
    assert set(hand.values()) == set(range(1, 10))
    for im, w in zip(ims, want):
        if im.name in hand:
            assert w == hand[im.name], im.name
    offs, total, got, status = run(ims)
    for im, s, w in zip(ims, status, want):
        assert (s == 0) == (w == 0), (im.name, s, w)
        if im.name in hand:
            assert s == hand[im.name], (im.name, s)
    assert status == want                                     # the Python statement of the decoder gives the same word
    covered = np.zeros(total, bool)
    for im, o, ref in zip(ims, offs, pixels):
        covered[o:o + im.out_bytes] = True
        if ref is not None:
            assert np.array_equal(got[o:o + ref.size].reshape(ref.shape), ref), im.name
    assert (got[~covered] == FILL).all(), "a guard byte was written"
    bad = png_cases.per_status()[6]
    with pytest.raises(RuntimeError, match="status6.*data exhausted"):
        png.decode([good, bad, good], "cuda")


def test_entry_point_refusals_launch_nothing():
    ims = [png_cases.build(9, 17, "rgb", "mix")[0], png_cases.build(6, 7, "gray16", "mix")[0]]
    sizes = [im.out_bytes for im in ims]
    pool, desc0 = png.descriptors(ims, [17, 1024])
    out = torch.full((1024 + sizes[1],), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((png.workspace_bytes(desc0),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call(d=None, which=0, **over):
        desc = (_lib.PngDesc * 2)()
        C.memmove(desc, desc0, C.sizeof(desc0))
        for k, v in (d or {}).items():
            setattr(desc[which], k, v)
        return launch(pool, desc, out, ws, status, desc_dev_table=desc0, **over)

    L.io_prof_begin_ex(0)
    refused = [
        (call(dict(H=0)), "size"), (call(dict(W=65536)), "size"), (call(dict(H=30000, W=30000)), "size"),
        (call(dict(channels=2)), "channels"), (call(dict(depth=4)), "channels"), (call(dict(depth=16)), "channels"),
        (call(dict(channels=3), which=1), "channels"),
        (call(dict(data_off=-1)), "data range"), (call(dict(data_bytes=-5)), "data range"),
        (call(dict(data_bytes=desc0[1].data_bytes + 1), which=1), "byte pool"), (call(pool_bytes=pool.size - 1), "byte pool"),
        (call(dict(out_off=-1)), "output"), (call(dict(out_off=1024 + 2), which=1), "output"),
        (call(out_bytes=1024 + sizes[1] - 1), "output"),
        (call(dict(out_off=1023), which=1), "2-byte aligned"),
        (call(n=0), "empty"), (call(n=65536), "65535"),
        (call(ws=ws.data_ptr() + 4), "aligned"),
        (call(out=0), "null"), (call(ws=0), "null"), (call(pool=0), "null"), (call(status=0), "null"), (call(desc_dev=0), "null"),
    ]
    for k, (rc, _) in enumerate(refused):
        assert rc == -1, (k, rc)
    assert call(desc_host=None) == -1
    assert call(ws_bytes=ws.numel() - 1) == -2 and "workspace" in _lib.last_error()        # IO_ERR_WORKSPACE
    assert call(dict(channels=2)) == -1 and "channels" in _lib.last_error()
    assert call(dict(out_off=1023), which=1) == -1 and "2-byte aligned" in _lib.last_error()
    assert call(dict(data_bytes=desc0[1].data_bytes + 1), which=1) == -1 and "byte pool" in _lib.last_error()
    assert call(out_bytes=1024 + sizes[1] - 1) == -1 and "output" in _lib.last_error()
    ent = (_lib.ProfEntry * 32)()
    assert L.io_prof_end(ent, 32) == 0, "a refused call launched something"
    assert bool((out == FILL).all()) and bool((ws == FILL).all()) and bool((status == -1).all())
    assert call() == 0, _lib.last_error()                       # and the tables as they are decode
    got = out.cpu().numpy()
    for (o, n), im in zip(((17, sizes[0]), (1024, sizes[1])), ims):
        assert np.array_equal(got[o:o + n], im.to_host().reshape(-1).view(np.uint8))
    assert (got[:17] == FILL).all() and (got[17 + sizes[0]:1024] == FILL).all()


def _as_png(a, name, **kw):
    return png_cases.build(a.shape[0], a.shape[1], "rgb", kw.pop("filters", "mix"), px=a, name=name, **kw)[0]


def test_renderer_png_equals_arrays_bit_for_bit():
    S = 64
    arrays, jp, masks, enc, items = _mixed_batch()
    pg = [_as_png(a, "image%d.png" % k) for k, a in enumerate(arrays)]
    rgba = png_cases.build(arrays[2].shape[0], arrays[2].shape[1], "rgba", 4, name="rgba.png",
                           px=np.concatenate([arrays[2], arrays[2][:, :, :1] // 2], 2))[0]
    want = [t.cpu().numpy() for t in datasets.PairRenderer(S, MEAN, STD).render(arrays, masks, items)]
    assert np.abs(want[0]).max() > 0 and want[1].any()
    r = datasets.PairRenderer(S, MEAN, STD)
    for name, ii, mm in (("png + dense masks", pg, masks), ("png + encoded masks", pg, enc),
                         ("array, jpeg and png + encoded masks", [pg[0], jp[1], arrays[2]], enc),
                         ("jpeg, png, rgba + dense masks", [jp[0], pg[1], rgba], masks)):
        got = r.render(ii, mm, items)
        for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
            assert np.array_equal(g.cpu().numpy(), w), (name, plane)
    r.render([pg[0], jp[1], arrays[2]], enc, items)
    assert r.last_upload["images"] == (arrays[2].size + len(pg[0].deflate_bytes()) + jp[1].nbytes_entropy
                                       + len(jp[1].tables_blob()))
    rgb0, m1, m2 = r.render(pg, enc, items, load_rgb=False)
    assert float(rgb0.abs().max()) == 0.0 and r.last_upload["images"] == 0
    assert np.array_equal(m1.cpu().numpy(), want[1]) and np.array_equal(m2.cpu().numpy(), want[2])
    r.check_status()
    # a batch without PNG images lays out and uploads what it did before
    r.render(jp, enc, items)
    with_jpeg = dict(r.last_upload)
    r2 = datasets.PairRenderer(S, MEAN, STD)
    r2.render(jp, enc, items)
    assert with_jpeg == r2.last_upload
    # a stream that does not decode is reported when its staging slot comes round again, or by check_status()
    broken = pg[0].with_stream(pg[0].deflate_bytes()[:40], name="broken.png")
    r.render([broken, pg[1], arrays[2]], enc, items)
    with pytest.raises(RuntimeError, match="broken.png"):
        r.check_status()
    r.render([broken, jp[1], arrays[2]], enc, items)
    r.render(pg, enc, items)
    with pytest.raises(RuntimeError, match="broken.png"):
        r.render(pg, enc, items)
    r.check_status()
    # a 16-bit depth map is no picture
    H, W = arrays[0].shape[:2]
    depth = png_cases.build(H, W, "gray16", "mix", name="depth.png")[0]
    with pytest.raises(ValueError, match="depth.png.*16-bit.*not a picture"):
        r.render([depth, pg[1], arrays[2]], masks, items)


class _PngReader(_JpegReader):
    """the 160 x 208 fixture image as a ``PngImage`` (``as_jpeg`` True) or as the array"""
    _png = []

    def load_image(self, image_fn):
        self.loads += 1
        a = jpeg_cases.load()[1][self.NAME][1]
        if not self._png:
            self._png.append(_as_png(a, "frame.png"))
        return self._png[0] if self._as_jpeg else a


def test_batches_over_a_png_reader_equal_the_array_reader():
    z = load_golden("dataset_items")
    cfg = dict(json.loads(str(z["config_json"])), patch_or_image="patch")
    outs = []
    for as_png in (False, True):
        rd = _PngReader(synthetic.SyntheticReader(int(z["reader_seed"])), as_png)
        ds = datasets.SupOcclusionOrderBatches(cfg, "train", "InstaOrderNet_o", rd, rd.load_image, rng=np.random.RandomState(101))
        outs.append(ds.batch(range(6)))
        ds.renderer.check_status()
    assert float(outs[0][0].abs().max()) > 0 and float(outs[0][1].abs().max()) > 0
    for f, (w, g) in enumerate(zip(*outs)):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w.cpu().numpy()), f
    assert ds.renderer.last_upload["images"] < 160 * 208 * 3 * 6


def test_prefetcher_reports_a_broken_file_at_its_end():
    z = load_golden("dataset_items")
    cfg = dict(json.loads(str(z["config_json"])), patch_or_image="patch")
    rd = _PngReader(synthetic.SyntheticReader(int(z["reader_seed"])), True)
    good = rd.load_image("x")
    rd.load_image = lambda fn: good.with_stream(good.deflate_bytes()[:100], name="half.png")
    ds = datasets.SupOcclusionOrderBatches(cfg, "train", "InstaOrderNet_o", rd, rd.load_image, rng=np.random.RandomState(5))
    pf = datasets.BatchPrefetcher(ds, [[0, 1], [2, 3]])
    with pytest.raises(RuntimeError, match="half.png"):
        for _ in pf:
            pass


def test_eval_dense_depth_png_device_equals_host(tmp_path):
    """three frames a few rows taller and wider than the 352 x 1216 crop, one entry without ground truth, a stub network
    (the smallest the dense-evaluation tests use): rows identical whether Pillow or io_png_decode reads the files"""
    from instaorder_amd import dense_eval
    from test_dense_eval_cpu import KITTI_DISP_SEED, KITTI_SEED
    from test_gpu_dense_eval import _StubNet
    lst = synthetic.write_mini_kitti(str(tmp_path), KITTI_SEED)
    assert all(352 < H < 352 + 40 and 1216 < W < 1216 + 40 for H, W in synthetic.MINI_KITTI_SIZES)
    disps = synthetic.dense_disparities(KITTI_DISP_SEED, 3, 352, 1216)
    rows = {}
    for mode in ("host", "device"):
        rd = dense_eval.KITTIEigenReader(lst, str(tmp_path), png=mode)
        present = [i for i in range(3) if rd.has_gt(i)]
        assert len(present) == 2
        img, box, gt = rd.load(present[0])
        assert png.is_png(img) == png.is_png(gt) == (mode == "device")
        if mode == "device":
            assert not img.raw16 and gt.raw16 and gt.shape == img.shape[:2]
        ren = dense_eval._renderer((352, 1216), MEAN, STD, torch.device("cuda", 0))
        rows["rgb " + mode] = dense_eval.render_rgb(ren, [img], [box]).cpu().numpy()
        ren.check_status()
        r = dense_eval.eval_dense_depth(_StubNet(disps[present]), rd, "midas_pretrained", batch=4, return_rows=True)
        assert r["missing"] == 1 and r["n_images"] == 2
        rows[mode] = r["rows"]
    assert rows["host"].shape == (2, 10) and np.isfinite(rows["host"]).all()
    assert rows["host"].tobytes() == rows["device"].tobytes()
    assert np.abs(rows["rgb host"]).max() > 0 and np.array_equal(rows["rgb host"], rows["rgb device"])
    with pytest.raises(ValueError, match="'host' or 'device'"):
        dense_eval.KITTIEigenReader(lst, str(tmp_path), png="gpu")


# ---- every region of the renderer's arena at once ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def everything():
    """Four images -- an array, a baseline JPEG file, a progressive one, a PNG file -- with dense masks, ``RLEMasks``,
    ``PolyMasks`` that hold polygons and a run-length instance, and dense masks again: every codec group of
    ``PairRenderer.render`` has members, beside uploaded arrays.  (arrays, dense masks, items, the planes of the batch as
    arrays and dense masks, make): ``make()`` builds the encoded batch under the settings of its moment."""
    import jpeg_prog_cases
    from instaorder_amd import jpeg, poly, rle
    base, prog = jpeg_cases.load()[1], jpeg_prog_cases.load()[1]
    names = ["21x35_444_q85", "40x24_422_q85", "33x47_420_q85", "33x47_420_lumafirst"]
    arrays = [base[names[0]][1], base[names[1]][1], prog[names[2]][1], prog[names[3]][1]]
    dense, items = [], []
    for ii, a in enumerate(arrays):
        H, W = a.shape[:2]
        y, x = np.mgrid[0:H, 0:W]
        dense.append(np.stack([(x > W // 4) & (y < 2 * H // 3), (x - W / 2) ** 2 + (y - H / 2) ** 2 < (min(H, W) / 3) ** 2,
                               (x + y) % 7 < 3]).astype(np.uint8))
        hw = max(H, W)
        items.append((ii, 0, 1, (W // 4 - 6, H // 4 - 5, 27, 27), datasets.INTER_CUBIC, bool(ii % 2)))
        items.append((ii, 1, 2, (-((hw - W) // 2), -((hw - H) // 2), hw, hw), datasets.INTER_LINEAR, not ii % 2))
        items.append((ii, 2, 0, (0, 0, W, H), datasets.INTER_LINEAR, False))
    H2, W2 = arrays[2].shape[:2]
    crowd = rle.RLEMasks.from_dense(dense[2][1:2]).counts[0]
    pm = poly.PolyMasks([[[2.5, 3.0, W2 - 3.0, 4.5, W2 / 2, H2 - 2.0]], {"size": [H2, W2], "counts": [int(c) for c in crowd]},
                         [[-4, -3, W2 + 2, H2 / 2, 3, H2 + 5], [1, 1, 5, 1, 5, 5]]], H2, W2, values=[1, 1, 9])
    assert pm.is_polygon(0) and not pm.is_polygon(1) and pm.is_polygon(2)
    dense[2] = pm.to_dense()
    assert all(m[i].any() for m in dense for i in range(3))

    def make():
        assert jpeg.get_progressive() == "device"
        images = [arrays[0], jpeg_cases.image(names[1]), jpeg.JpegImage(prog[names[2]][0], name=names[2]),
                  _as_png(arrays[3], "image3.png")]
        assert images[2].progressive and images[2].supported and not images[1].progressive
        return images, [dense[0], rle.RLEMasks.from_dense(dense[1] != 0), pm, dense[3]]

    want = [t.cpu().numpy() for t in datasets.PairRenderer(64, MEAN, STD).render(arrays, dense, items)]
    assert np.abs(want[0]).max() > 0 and want[1].any() and want[2].any()
    return arrays, dense, items, want, make


@pytest.fixture
def device_progressive():
    from instaorder_amd import jpeg
    was = dict(jpeg._PROGRESSIVE)
    jpeg.set_progressive("device")
    yield
    jpeg.set_progressive(was["mode"], was["concurrent"])


@pytest.mark.parametrize("stages", ["sequential", "parallel"])
def test_renderer_with_every_region_non_empty_equals_arrays(everything, device_progressive, stages):
    """all five codec groups, uploaded arrays and dense masks in one batch, under both entropy and both inflate stages:
    the three planes are those of the batch as arrays and dense masks, bit for bit"""
    from instaorder_amd import jpeg
    arrays, dense, items, want, make = everything
    was_e, was_i = jpeg.get_entropy(), png.get_inflate()
    try:
        jpeg.set_entropy(stages, was_e["subseq_bytes"], was_e["max_rounds"])
        png.set_inflate(stages, was_i["chunk_bytes"])
        images, masks = make()
        r = datasets.PairRenderer(64, MEAN, STD)
        for turn in range(3):                                    # both staging slots, and the first one again
            got = r.render(images, masks, items)
            for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
                assert np.array_equal(g.cpu().numpy(), w), (stages, turn, plane)
        r.check_status()
    finally:
        jpeg.set_entropy(was_e["mode"], was_e["subseq_bytes"], was_e["max_rounds"])
        png.set_inflate(was_i["mode"], was_i["chunk_bytes"])
    up = r.last_upload
    assert up["images"] > arrays[0].size and up["masks"] > dense[0].size + dense[3].size
    assert up["total"] >= up["images"] + up["masks"] + up["descriptors"]


def test_renderer_with_empty_image_regions(everything, device_progressive):
    """the same batch without its images: no image is uploaded or decoded, the masks are the same and rgb is zero"""
    arrays, dense, items, want, make = everything
    images, masks = make()
    r = datasets.PairRenderer(64, MEAN, STD)
    for ims in (images, [None] * len(images)):
        rgb, m1, m2 = r.render(ims, masks, items, load_rgb=False)
        assert r.last_upload["images"] == 0
        assert tuple(rgb.shape) == want[0].shape and float(rgb.abs().max()) == 0.0
        assert np.array_equal(m1.cpu().numpy(), want[1]) and np.array_equal(m2.cpu().numpy(), want[2])
    r.check_status()


def test_renderer_reports_a_failure_of_one_codec_beside_healthy_ones(everything, device_progressive):
    """a truncated PNG stream in one batch, a truncated baseline scan in the next, both beside the healthy members of the
    other groups: the first is named when its staging slot comes round, the second by check_status(); a rejected stream
    is a status word, and the renderer goes on"""
    arrays, dense, items, want, make = everything
    images, masks = make()
    bad_png = images[3].with_stream(images[3].deflate_bytes()[:40], name="truncated.png")
    bad_jpg = images[1].with_entropy(images[1].entropy_bytes()[:40], "truncated.jpg")
    r = datasets.PairRenderer(64, MEAN, STD)
    r.render(images[:3] + [bad_png], masks, items)
    r.render([images[0], bad_jpg] + images[2:], masks, items)
    with pytest.raises(RuntimeError, match="PNG decode failed: truncated.png") as e:
        r.render(images, masks, items)
    assert "truncated.jpg" not in str(e.value)
    with pytest.raises(RuntimeError, match="JPEG decode failed: truncated.jpg") as e:
        r.check_status()
    assert "truncated.png" not in str(e.value)
    got = r.render(images, masks, items)
    for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
        assert np.array_equal(g.cpu().numpy(), w), plane
    r.check_status()
