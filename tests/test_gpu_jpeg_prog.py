"""Progressive JPEG files on the MI355X: io_jpeg_decode_prog_u8 (csrc/jpeg.hip, csrc/jpeg_prog.h) byte for byte against what
the reference's ``Image.open(f).convert('RGB')`` made of the fixture files (tests/golden/jpeg_prog_cases.npz), with the scans
of a level side by side and with all scans on one lane; guard bytes; damaged scans against the lines of the host program
tests/jpeg_prog_host.cpp; the renderer on a batch that mixes progressive files, baseline files and arrays; the refusals."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import jpeg_cases
import jpeg_prog_cases as cases
from helpers import ROOT
from instaorder_amd import _lib, datasets, jpeg

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
GUARD, FILL = 48, 0xAB
NAMES, CASES, _ = cases.load()
BASE_NAMES, BASE_CASES, _ = jpeg_cases.load()


def upload(a):
    a = np.frombuffer(a, dtype=np.uint8) if not isinstance(a, np.ndarray) else a
    return torch.from_numpy(a.copy() if a.size else np.zeros(16, np.uint8)).cuda()


def launch(p, t_out, t_ws, t_status, concurrent=1, dev=None, **over):
    """io_jpeg_decode_prog_u8 on the tables ``p`` of jpeg.descriptors_progressive (device copies from ``dev``, another such
    dict, when given: the host tables of a refused call differ from what is on the device); ``over`` replaces arguments"""
    keep = [upload(b) for b in jpeg.progressive_blobs(dev or p)]          # tables, huff, desc, image, scan, pool
    a = dict(pool=keep[5].data_ptr(), pool_bytes=p["pool"].size, tables_dev=keep[0].data_ptr(),
             tables_host=p["tables"].ctypes.data_as(C.c_void_p), tables_bytes=p["tables"].size, huff_dev=keep[1].data_ptr(),
             huff_host=p["huff"].ctypes.data_as(C.c_void_p), n_huff=p["huff"].size // 272, desc_dev=keep[2].data_ptr(),
             desc_host=C.cast(p["desc"], C.c_void_p), image_dev=keep[3].data_ptr(), image_host=C.cast(p["image"], C.c_void_p),
             n=len(p["desc"]), scan_dev=keep[4].data_ptr(), scan_host=C.cast(p["scan"], C.c_void_p), n_scans=p["n_scans"],
             out=t_out.data_ptr(), out_bytes=t_out.numel(), ws=t_ws.data_ptr(), ws_bytes=t_ws.numel(), status=t_status.data_ptr(),
             concurrent=concurrent)
    a.update(over)
    rc = _lib.lib().io_jpeg_decode_prog_u8(
        C.c_void_p(a["pool"]), C.c_size_t(a["pool_bytes"]), C.c_void_p(a["tables_dev"]), a["tables_host"],
        C.c_size_t(a["tables_bytes"]), C.c_void_p(a["huff_dev"]), a["huff_host"], a["n_huff"], C.c_void_p(a["desc_dev"]),
        a["desc_host"], C.c_void_p(a["image_dev"]), a["image_host"], a["n"], C.c_void_p(a["scan_dev"]), a["scan_host"],
        a["n_scans"], C.c_void_p(a["out"]), C.c_size_t(a["out_bytes"]), C.c_void_p(a["ws"]), C.c_size_t(a["ws_bytes"]),
        C.c_void_p(a["status"]), a["concurrent"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
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


def coefficient_checksums(p, ws):
    """the host program's checksum over each image's coefficient range of the workspace (offsets | derived tables |
    coefficients, 128 bytes per block | planes | scan status: include/instaorder_hip.h)"""
    n = len(p["desc"])
    at = ((n + 1) * 8 + 15 & ~15) + (p["huff"].size // 272 * 904 + 15 & ~15)
    raw = ws.cpu().numpy()
    sums = []
    for d in p["desc"]:
        blocks = -(-d.W // (8 * d.hs)) * -(-d.H // (8 * d.vs)) * (d.hs * d.vs + (2 if d.n_comp == 3 else 0))
        sums.append(cases.checksum(raw[at:at + 128 * blocks].view(np.int16)))
        at += 128 * blocks
    return sums


def test_decode_mixed_with_baseline_byte_exact_both_ways():
    """every progressive fixture -- 1x1 to 96x136, 4:4:4 / 4:2:2 / 4:2:0 / grayscale, qualities 20 to 100, restart intervals,
    reordered scans -- and a baseline file between every three of them in ONE jpeg.decode call: byte-equal to the stored
    arrays with the scans of a level side by side (concurrent 1) and with all scans on one lane (0)"""
    ims, want = [], []
    for k, name in enumerate(NAMES):
        ims.append(cases.image(name))
        want.append(CASES[name][1])
        if k % 3 == 0:
            b = BASE_NAMES[(7 * k) % len(BASE_NAMES)]
            ims.append(jpeg_cases.image(b))
            want.append(BASE_CASES[b][1])
    assert sum(im.progressive for im in ims) == len(NAMES) and sum(not im.progressive for im in ims) >= 10
    for concurrent in (1, 0):
        got = jpeg.decode(ims, "cuda", concurrent=concurrent)
        for im, g, w in zip(ims, got, want):
            g = g.cpu().numpy()
            assert g.shape == w.shape and np.array_equal(g, w), "%s (concurrent %d): %d of %d bytes differ" % (
                im.name, concurrent, (g != w).sum(), w.size)
    # progressive images alone, and the parallel baseline stage next to them
    got = jpeg.decode(ims[-3:], "cuda", entropy="parallel")
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want[-3:]))
    with pytest.raises(ValueError, match="not supported"):
        jpeg.decode([jpeg.JpegImage(CASES[NAMES[0]][0])], "cuda")


def test_direct_call_writes_no_byte_outside_an_image():
    ims = [cases.image(n) for n in NAMES]
    offs, total = offsets(ims)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    p = jpeg.descriptors_progressive(ims, offs)
    expect = np.full(total, FILL, np.uint8)
    for name, o in zip(NAMES, offs):
        expect[o:o + CASES[name][1].size] = CASES[name][1].reshape(-1)
    ws = torch.full((jpeg.workspace_bytes_progressive(p),), FILL, dtype=torch.uint8, device="cuda")
    sums = None
    for concurrent in (1, 0, 1):                                 # the third call on the used workspace
        out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
        assert launch(p, out, ws, status, concurrent=concurrent) == 0, _lib.last_error()
        assert status.cpu().numpy().tolist() == [0] * len(ims)
        got = out.cpu().numpy()
        for name, o in zip(NAMES, offs):
            ref = CASES[name][1]
            g = got[o:o + ref.size].reshape(ref.shape)
            assert np.array_equal(g, ref), "%s (concurrent %d): %d of %d bytes differ" % (name, concurrent, (g != ref).sum(), ref.size)
        assert np.array_equal(got, expect), "a guard byte was written"
        if sums is None:
            sums = coefficient_checksums(p, ws)
            assert sums[:4] == [cases.checksum(im.coefficients()) for im in ims[:4]]
        else:
            assert coefficient_checksums(p, ws) == sums


@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    """the lines of tests/jpeg_prog_host.cpp for three fixture images (built without the sanitizers here: the runs under them
    are tests/test_jpeg_prog_cpu.py)"""
    names = ["21x35_420_rst2", "33x47_444_q85", "40x24_gray_rst2"]
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    tmp = tmp_path_factory.mktemp("jpeg_prog_host")
    exe = str(tmp / "jpeg_prog_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "instaorder_amd", "csrc"),
                    os.path.join(ROOT, "tests", "jpeg_prog_host.cpp"), "-o", exe], check=True, capture_output=True)
    files = []
    for k, n in enumerate(names):
        files.append(str(tmp / ("image%d.bin" % k)))
        with open(files[-1], "wb") as f:
            f.write(cases.image_file(cases.image(n)))
    run = subprocess.run([exe] + files, check=True, capture_output=True, text=True)
    return names, [ln.split() for ln in run.stdout.splitlines()]


def test_damaged_scans_give_the_host_programs_status_and_coefficients(host_rows):
    """truncations and mutations of single scans that the host program ran, each between intact images in one call: status
    word and coefficient checksum are the host program's, the neighbours are byte exact, guard bytes stay, the result does
    not depend on ``concurrent``, and jpeg.decode raises naming the image"""
    names, rows = host_rows
    ims, want, pixels = [], [], []
    for s, name in enumerate(names):
        base = cases.image(name)
        for n in (0, 1, len(base.scans) - 5, len(base.scans) - 1):        # DC first, AC first, an AC refinement, the last refinement
            mine = [r for r in rows if int(r[0]) == s and int(r[2]) == n]
            cuts = [r for r in mine if r[1] == "T"]
            picked = [cuts[0], cuts[len(cuts) // 3], cuts[-1]] + [r for r in mine if r[1] == "M"][4 * s:4 * s + 3]
            for r in picked:
                data = base.scan_bytes(n)
                data = data[:int(r[3])] if r[1] == "T" else cases.mutated(data, int(r[3]))
                ims += [base, base.with_scan(n, data, "%s scan %d %s %s" % (name, n, r[1], r[3]))]
                want += [(0, None), (int(r[4]), int(r[5]))]
                pixels += [CASES[name][1], None]
    assert sum(1 for w in want if w[0]) >= 30 and len({w[0] for w in want}) >= 4
    offs, total = offsets(ims)
    p = jpeg.descriptors_progressive(ims, offs)
    ws = torch.empty(jpeg.workspace_bytes_progressive(p), dtype=torch.uint8, device="cuda")
    for concurrent in (1, 0):
        out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        status = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
        assert launch(p, out, ws, status, concurrent=concurrent) == 0, _lib.last_error()
        assert status.cpu().numpy().tolist() == [w[0] for w in want]
        sums = coefficient_checksums(p, ws)
        for im, w, got in zip(ims, want, sums):
            assert w[1] is None or got == w[1], (im.name, concurrent)
        got = out.cpu().numpy()
        covered = np.zeros(total, bool)
        for im, o, ref in zip(ims, offs, pixels):
            n = im.H * im.W * 3
            covered[o:o + n] = True
            if ref is not None:
                assert np.array_equal(got[o:o + n].reshape(ref.shape), ref), (im.name, concurrent)
        assert (got[~covered] == FILL).all(), "a guard byte was written"
    bad = next(im for im, w in zip(ims, want) if w[0])
    with pytest.raises(RuntimeError, match="scan 0 T 0"):
        jpeg.decode([ims[0], bad, jpeg_cases.image("9x17_420_q85")], "cuda")


def test_renderer_on_progressive_baseline_and_arrays_equals_arrays():
    S = 64
    names = ["33x47_420_q85", "40x24_422_q85", "21x35_444_q85", "33x47_420_lumafirst"]
    arrays = [CASES[names[0]][1], BASE_CASES[names[1]][1], BASE_CASES[names[2]][1], CASES[names[3]][1]]
    mixed = [cases.image(names[0]), jpeg_cases.image(names[1]), arrays[2], cases.image(names[3])]
    masks, items = [], []
    for ii, a in enumerate(arrays):
        H, W = a.shape[:2]
        y, x = np.mgrid[0:H, 0:W]
        masks.append(np.stack([(x > W // 4) & (y < 2 * H // 3), (x - W / 2) ** 2 + (y - H / 2) ** 2 < (min(H, W) / 3) ** 2,
                               (x + y) % 7 < 3]).astype(np.uint8))
        hw = max(H, W)
        items.append((ii, 0, 1, (W // 4 - 6, H // 4 - 5, 27, 27), datasets.INTER_CUBIC, bool(ii % 2)))
        items.append((ii, 1, 2, (-((hw - W) // 2), -((hw - H) // 2), hw, hw), datasets.INTER_LINEAR, not ii % 2))
    want = [t.cpu().numpy() for t in datasets.PairRenderer(S, MEAN, STD).render(arrays, masks, items)]
    assert np.abs(want[0]).max() > 0 and want[1].any()
    r = datasets.PairRenderer(S, MEAN, STD)
    try:
        for mode in ("sequential", "parallel"):                  # set_entropy applies to the baseline image only
            jpeg.set_entropy(mode)
            got = r.render(mixed, masks, items)
            for g, w, plane in zip(got, want, ("rgb", "modal1", "modal2")):
                assert np.array_equal(g.cpu().numpy(), w), (mode, plane)
            r.check_status()
    finally:
        jpeg.set_entropy("sequential")
    up = r.last_upload
    assert arrays[2].size < up["images"] < sum(a.size for a in arrays)
    # a progressive file with a damaged scan is reported like a baseline one
    broken = mixed[0].with_scan(4, mixed[0].scan_bytes(4)[:10], "broken_progressive.jpg")
    r.render([broken] + mixed[1:], masks, items)
    with pytest.raises(RuntimeError, match="broken_progressive.jpg"):
        r.check_status()


def test_entry_point_refusals_launch_nothing():
    ims = [cases.image(n) for n in ("9x17_420_q85", "21x35_gray_q85")]
    sizes = [im.H * im.W * 3 for im in ims]
    p0 = jpeg.descriptors_progressive(ims, [16, 1024])
    out = torch.full((1024 + sizes[1],), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((jpeg.workspace_bytes_progressive(p0),), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    L = _lib.lib()
    assert [s.level for s in p0["scan"]][:10] == [0, 1, 1, 1, 1, 2, 1, 2, 2, 3]

    def call(scan=None, which=0, desc=None, image=None, table=None, **over):
        p = dict(p0)
        for key, cls, change in (("scan", _lib.JpegProgScan, scan), ("desc", _lib.JpegDesc, desc), ("image", _lib.JpegProgImage, image)):
            arr = (cls * len(p0[key]))()
            C.memmove(arr, p0[key], C.sizeof(p0[key]))
            for k, v in (change or {}).items():
                if isinstance(v, tuple):
                    getattr(arr[which], k)[v[0]] = v[1]
                else:
                    setattr(arr[which], k, v)
            p[key] = arr
        p["huff"] = p0["huff"].copy()
        if table is not None:
            p["huff"][table[0]] = table[1]
        return launch(p, out, ws, status, dev=p0, **over)

    L.io_prof_begin_ex(0)
    ac = p0["scan"][1].table[0]                                  # the AC table of scan 1
    refused = [
        # the image descriptors, as for io_jpeg_decode_u8
        (call(desc=dict(hs=1, vs=2)), "sampling"), (call(desc=dict(n_comp=4)), "components"), (call(desc=dict(H=0)), "size"),
        (call(desc=dict(table_set=-1)), "table set"), (call(desc=dict(quant=(1, 4))), "quant"),
        (call(desc=dict(out_off=-1)), "output"), (call(desc=dict(out_off=1024 + 1), which=1), "output"),
        (call(out_bytes=1024 + sizes[1] - 1), "output"), (call(tables_bytes=jpeg.TABLES_BYTES - 1), "table set"),
        (call(n=0), "empty"),
        # the scan ranges of the images
        (call(image=dict(first_scan=1)), "ranges"), (call(image=dict(n_scans=17)), "ranges"),
        (call(image=dict(n_scans=9)), "incomplete progression"),             # the last luma refinement left out
        (call(image=dict(n_levels=0)), "n_levels"), (call(image=dict(n_levels=11)), "n_levels"), (call(n_scans=15), "ranges"),
        (call(n_scans=0), "n_scans"), (call(n_huff=0), "n_huff"), (call(scan=dict(image=1), which=3), "names image"),
        # the fields of a scan
        (call(scan=dict(n_comp=0), which=1), "components"), (call(scan=dict(n_comp=2), which=0), "components"),
        (call(scan=dict(comp=(0, 3)), which=1), "frame order"), (call(scan=dict(comp=(1, 0)), which=0), "frame order"),
        (call(scan=dict(se=64), which=1), "Ss="), (call(scan=dict(ss=6), which=1), "Ss="), (call(scan=dict(se=1), which=0), "Ss="),
        (call(scan=dict(n_comp=3, ss=1, se=1), which=0), "Ss="),
        (call(scan=dict(al=14), which=1), "Al <= 13"), (call(scan=dict(ah=4), which=1), "Ah 0 or Al + 1"),
        (call(scan=dict(restart_interval=-1), which=2), "restart_interval"),
        (call(scan=dict(level=-1), which=2), "level"), (call(scan=dict(level=4), which=9), "level"),
        # the scan rules
        (call(scan=dict(ss=0, se=0), which=1), "a first scan: not sent before"),             # the DC a second time
        (call(scan=dict(ah=3), which=1), "a refinement: Ah = the previous Al"),             # a refinement of what was never sent
        (call(scan=dict(ah=2, al=1), which=9), "a refinement: Ah = the previous Al"),       # a bit sent twice
        (call(scan=dict(comp=(0, 1)), which=1), "a first scan: not sent before"),           # luma 1..5 sent for Cb instead ...
        (call(scan=dict(ah=0, al=1), which=5), "a first scan: not sent before"),
        (call(scan=dict(al=1, ah=0), which=9), "a first scan: not sent before"),
        (call(scan=dict(ss=2), which=1), "a refinement: Ah = the previous Al"),             # coefficient 1 never sent, then refined
        (call(scan=dict(se=62), which=4), "a refinement: Ah = the previous Al"),
        (call(scan=dict(al=1, ah=2), which=9), "a refinement"),
        (call(scan=dict(ss=1, se=5, n_comp=1), which=0), "in front of its first DC scan"),
        # tables and data
        (call(scan=dict(table=(0, -1)), which=1), "outside the pool"), (call(scan=dict(table=(2, 999)), which=0), "outside the pool"),
        (call(table=(272 * ac, 3)), "prefix code"), (call(table=(272 * ac + 15, 255)), "prefix code"),
        (call(scan=dict(data_off=-1), which=3), "byte pool"), (call(scan=dict(data_bytes=-2), which=3), "byte pool"),
        (call(scan=dict(data_bytes=p0["scan"][15].data_bytes + 1), which=15), "byte pool"),
        (call(pool_bytes=p0["pool"].size - 1), "byte pool"),
        # the level rule: a refinement on the level of the scan it refines, or below it
        (call(scan=dict(level=1), which=5), "not above level"), (call(scan=dict(level=0), which=6), "not above level"),
        (call(scan=dict(level=2), which=9), "not above level"), (call(scan=dict(level=0), which=15), "not above level"),
        (call(concurrent=2), "concurrent"), (call(ws=ws.data_ptr() + 4), "aligned"),
        (call(out=0), "null"), (call(ws=0), "null"), (call(pool=0), "null"), (call(status=0), "null"), (call(huff_dev=0), "null"),
        (call(huff_host=None), "null"), (call(image_dev=0), "null"), (call(scan_host=None), "null"), (call(desc_dev=0), "null"),
    ]
    for k, (rc, _) in enumerate(refused):
        assert rc == -1, (k, rc)
    assert call(ws_bytes=ws.numel() - 1) == -2 and "workspace" in _lib.last_error()        # IO_ERR_WORKSPACE
    for kw, why in ((dict(scan=dict(level=1), which=5), "not above level 1"), (dict(scan=dict(al=14), which=1), "Al <= 13"),
                    (dict(image=dict(n_scans=9)), "incomplete progression: coefficient 1 of component 0 is not refined down to Al = 0"),
                    (dict(scan=dict(ss=1, se=5, n_comp=1), which=0), "in front of its first DC scan"),
                    (dict(table=(272 * ac, 3)), "prefix code"), (dict(image=dict(first_scan=1)), "ranges"),
                    (dict(scan=dict(table=(0, -1)), which=1), "outside the pool")):
        assert call(**kw) == -1 and why in _lib.last_error(), (why, _lib.last_error())
    ent = (_lib.ProfEntry * 32)()
    assert L.io_prof_end(ent, 32) == 0, "a refused call launched something"
    assert bool((out == FILL).all()) and bool((ws == FILL).all()) and bool((status == -1).all())
    # a level assignment other than scan_levels() that keeps the rule is taken: every scan on a level of its own
    serial = dict(p0)
    for key, cls in (("scan", _lib.JpegProgScan), ("image", _lib.JpegProgImage)):
        serial[key] = (cls * len(p0[key]))()
        C.memmove(serial[key], p0[key], C.sizeof(p0[key]))
    for k in range(10):
        serial["scan"][k].level = k
    serial["image"][0].n_levels = 10
    assert launch(serial, out, ws, status) == 0, _lib.last_error()
    got = out.cpu().numpy()
    assert status.cpu().numpy().tolist() == [0, 0]
    for (o, n), name in zip(((16, sizes[0]), (1024, sizes[1])), ("9x17_420_q85", "21x35_gray_q85")):
        assert np.array_equal(got[o:o + n], CASES[name][1].reshape(-1))
    assert (got[:16] == FILL).all() and (got[16 + sizes[0]:1024] == FILL).all()
