"""PNG files on the host: the parser, ``PngImage.to_host()`` (the contract of the kernels) against what Pillow made of the
fixture files and against files built here with every property forced, unsupported files naming their reason, the loader's
dispatch and fall-back, the ABI declarations, and the inflate loop the kernel compiles (csrc/png_inflate.h) built for the
CPU and run under the sanitizers on intact, truncated, mutated and hand-made streams.  All comparisons are exact; nothing
here needs a GPU or Pillow (one test uses Pillow if it is there)."""
import ctypes as C
import io
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_cases
from helpers import ROOT
from instaorder_amd import _lib, png

NAMES, CASES, UNSUPPORTED = png_cases.load()


def test_parser_fields_of_every_fixture():
    assert len(NAMES) == len(set(NAMES)) >= 12
    forms = set()
    for name in NAMES:
        data, ref = CASES[name]
        im = png.PngImage(data, name=name)
        m = re.match(r"(\d+)x(\d+)_(rgba|rgb|gray16|gray)", name)
        H, W, form = int(m.group(1)), int(m.group(2)), m.group(3)
        forms.add(form)
        ct, depth, ch = png_cases.FORMS[form]
        assert im.supported and im.reason is None, (name, im.reason)
        assert (im.H, im.W, im.colour_type, im.bit_depth, im.channels) == (H, W, ct, depth, ch)
        assert im.shape == ref.shape == ((H, W) if form == "gray16" else (H, W, 3)) and im.ndim == ref.ndim
        assert im.dtype == ref.dtype == (np.uint16 if form == "gray16" else np.uint8)
        assert im.raw16 == (form == "gray16")
        assert im.nbytes_compressed == len(data)
        assert im.nbytes_stream == sum(L for t, L in im.chunks if t == "IDAT") == len(im.deflate_bytes()) + 6
        assert zlib.adler32(zlib.decompress(data[data.index(b"IDAT") + 4:][:im.nbytes_stream])) == im.adler
        assert im.inflated_bytes == H * (1 + W * ch * depth // 8)
        assert png.is_png(im) and not png.is_png(ref)
    assert forms == {"rgb", "rgba", "gray", "gray16"}
    chunks = {t for n in NAMES for t, _ in png.PngImage(CASES[n][0]).chunks}
    assert {"tRNS", "gAMA"} <= chunks
    # the same through bytearray / memoryview, and with bytes behind IEND
    data, ref = CASES[NAMES[2]]
    for d in (bytearray(data), memoryview(data), data + b"trailing bytes"):
        assert np.array_equal(png.PngImage(d).to_host(), ref)


def test_to_host_equals_pillow_on_every_fixture():
    for name in NAMES:
        data, ref = CASES[name]
        got = png.PngImage(data, name=name).to_host()
        assert got.dtype == ref.dtype and got.shape == ref.shape, name
        assert np.array_equal(got, ref), "%s: %d of %d values differ" % (name, (got != ref).sum(), ref.size)


def test_to_host_on_built_files():
    for im, want in png_cases.batch_cases():
        got = im.to_host()
        assert got.dtype == want.dtype and np.array_equal(got, want), im.name
    for im, want, check in png_cases.stream_cases():
        assert check(im.stream_stats()), (im.name, im.stream_stats())
        assert np.array_equal(im.to_host(), want), im.name


def test_built_files_are_what_pillow_reads():
    Image = pytest.importorskip("PIL.Image")
    for im, want in png_cases.batch_cases()[:12] + [c[:2] for c in png_cases.stream_cases()[3:8]]:
        img = Image.open(io.BytesIO(im.data))
        ref = np.array(img) if im.raw16 else np.array(img.convert("RGB"))
        assert ref.dtype == want.dtype and np.array_equal(ref, want), im.name


def test_stream_stats_counts():
    im, _ = png_cases.build(20, 30, "rgb", 0, level=0)
    st = im.stream_stats()
    assert st == dict(stored=1, fixed=0, dynamic=0, min_distance=0, max_distance=0, max_length=0, overlapping=0,
                      max_code_length=0, output_bytes=20 * 91, status=0)
    im, _ = png_cases.distance_32768()
    st = im.stream_stats()
    assert (st["stored"], st["fixed"], st["min_distance"], st["max_distance"], st["max_length"]) == (1, 1, 32768, 32768, 258)
    assert st["output_bytes"] == 65536 and st["max_code_length"] == 8


def test_unsupported_files_say_why():
    want = {"palette": "palette", "interlaced": "Adam7", "rgb16": "16-bit colour", "4bit_gray": "4-bit"}
    assert set(UNSUPPORTED) == set(want)
    for kind, data in UNSUPPORTED.items():
        im = png.PngImage(data, name=kind)
        assert not im.supported and want[kind] in im.reason, (kind, im.reason)
        assert (im.H, im.W) == (21, 35)
        with pytest.raises(ValueError, match="not supported"):
            im.to_host()
        with pytest.raises(ValueError, match="not supported"):
            png.descriptors([im], [0])

    def header(W, H, depth=8, ct=2):
        return png_cases.png_file(H, W, "rgb", zlib.compress(b"\0" * 8)).replace(
            struct.pack(">IIBB", W, H, 8, 2), struct.pack(">IIBB", W, H, depth, ct))

    def recrc(data):
        body = data[12:29]
        return data[:29] + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF) + data[33:]

    for d, why in [(header(70000, 3), "above 65535"), (header(3, 65536), "above 65535"), (header(30000, 30000), "2^31"),
                   (header(5, 5, 8, 4), "gray with alpha"), (header(5, 5, 2, 0), "2-bit"), (header(5, 5, 16, 6), "16-bit colour")]:
        im = png.PngImage(recrc(d))
        assert not im.supported and why in im.reason, (why, im.reason)


def test_broken_files_raise():
    im, _ = png_cases.build(6, 7, "rgb", "mix")
    data = im.data
    idat = data.index(b"IDAT")
    flip = lambda at: data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]
    bad_header = bytearray(data)
    bad_header[idat + 4] = 0x79                             # CM = 9
    body = bytes(bad_header[idat:idat + 4 + im.nbytes_stream])
    bad_header[idat + 4 + im.nbytes_stream:idat + 8 + im.nbytes_stream] = struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
    for bad in (b"", b"\x89PNG", b"\xff\xd8" + data, data[:20], data[:idat + 10], flip(20), flip(idat + 9),
                data[:33] + data[idat + im.nbytes_stream + 8:], data[:8] + data[33:], bytes(bad_header)):
        with pytest.raises(ValueError):
            png.PngImage(bad)
    # a damaged ancillary chunk is ignored, as the chunk is
    anc, want = png_cases.batch_cases()[-1]
    at = anc.data.index(b"gAMA") + 5
    assert np.array_equal(png.PngImage(anc.data[:at] + b"\x55" + anc.data[at + 1:]).to_host(), want)


def test_damaged_streams_are_flagged_with_their_status():
    for status, im in png_cases.per_status().items():
        if status == 0:
            im.to_host()
            continue
        with pytest.raises(png.PngStreamError) as e:
            im.to_host()
        assert e.value.status == status and png.STATUS[status] in str(e.value), (status, e.value)
    for im, status in png_cases.more_statuses():
        with pytest.raises(png.PngStreamError) as e:
            im.to_host()
        assert e.value.status == status, (im.name, e.value)


def test_loader_dispatch_and_fallback(tmp_path):
    import jpeg_cases
    from instaorder_amd import jpeg
    ok, rgb = CASES["7x5_rgb"]
    (tmp_path / "a.png").write_bytes(ok)
    (tmp_path / "d.png").write_bytes(CASES["30x41_gray16"][0])
    (tmp_path / "p.png").write_bytes(UNSUPPORTED["palette"])
    (tmp_path / "j.jpg").write_bytes(jpeg_cases.load()[1]["16x16_420_q85"][0])
    (tmp_path / "n.bin").write_bytes(b"neither")
    (tmp_path / "t.png").write_bytes(ok[:40])
    seen = []

    def fallback(path):
        seen.append(os.path.basename(path))
        return np.zeros((21, 35, 3), np.uint8)

    load = png.loader(str(tmp_path), fallback=fallback)
    a = load("a.png")
    assert png.is_png(a) and a.supported and a.name == "a.png" and np.array_equal(a.to_host(), rgb) and not seen
    j = load("j.jpg")
    assert jpeg.is_jpeg(j) and j.supported and not seen
    for fn in ("d.png", "p.png", "n.bin", "t.png"):          # a 16-bit depth map is no picture: the fallback decides
        assert load(fn).shape == (21, 35, 3)
    assert seen == ["d.png", "p.png", "n.bin", "t.png"]
    assert isinstance(png.loader(str(tmp_path), jpeg=False, fallback=fallback)("j.jpg"), np.ndarray) and seen[-1] == "j.jpg"
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="Pillow"):
            png.loader(str(tmp_path))("p.png")
    else:
        got = png.loader(str(tmp_path))("p.png")
        assert isinstance(got, np.ndarray) and got.shape == (21, 35, 3) and got.dtype == np.uint8


def test_kitti_reader_png_switch(tmp_path, monkeypatch):
    from instaorder_amd import dense_eval
    lst = tmp_path / "eigen_test.txt"
    lst.write_text("a/b.png None 721.5\n")
    monkeypatch.delenv("IO_KITTI_PNG", raising=False)
    assert dense_eval.KITTIEigenReader(str(lst), str(tmp_path)).png == "host"
    assert dense_eval.KITTIEigenReader(str(lst), str(tmp_path), -1, "device").png == "device"
    monkeypatch.setenv("IO_KITTI_PNG", "device")
    assert dense_eval.KITTIEigenReader(str(lst), str(tmp_path)).png == "device"
    assert dense_eval.KITTIEigenReader(str(lst), str(tmp_path), png="host").png == "host"      # the argument decides
    monkeypatch.setenv("IO_KITTI_PNG", "gpu")
    with pytest.raises(ValueError, match="IO_KITTI_PNG"):
        dense_eval.KITTIEigenReader(str(lst), str(tmp_path))
    # a frame and a ground truth the device takes come back as PngImage objects, anything else as today's arrays
    frame, _ = png_cases.build(360, 1220, "rgb", 1, seed=3)
    depth, _ = png_cases.build(360, 1220, "gray16", 0, seed=4)
    for sub, rel, data in (("rawdata", "a/b.png", frame.data), ("data_depth_annotated", "c.png", depth.data),
                           ("rawdata", "a/p.png", png_cases.build(360, 1220, "gray16", 0, seed=5)[0].data)):
        p = tmp_path / sub / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(data)
    lst.write_text("a/b.png c.png 721.5\n")
    img, box, gt = dense_eval.KITTIEigenReader(str(lst), str(tmp_path), png="device").load(0)
    assert png.is_png(img) and not img.raw16 and png.is_png(gt) and gt.raw16 and box == (2, 8, 1216, 352)
    assert dense_eval._device_png(str(tmp_path / "rawdata" / "a/p.png"), False) is None      # 16-bit gray is no frame
    assert dense_eval._device_png(str(lst), True) is None                                  # not a PNG at all


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    for name, nargs in (("io_png_decode", 11), ("io_png_workspace_bytes", 2)):
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name + " is not declared in include/instaorder_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert "} io_png_desc;" in hdr
    assert C.sizeof(_lib.PngDesc) == 48
    fields = re.search(r"typedef struct io_png_desc \{(.*?)\} io_png_desc;", hdr, re.S).group(1)
    names = [n.split("[")[0] for ln in fields.splitlines() for n in re.findall(r"(\w+(?:\[\d+\])?)\s*[,;]", ln.split("/*")[0])]
    assert names == [f[0] for f in _lib.PngDesc._fields_]
    lib = _lib.lib()
    assert hasattr(lib, "io_png_decode") and hasattr(lib, "io_png_workspace_bytes")
    assert lib.io_abi_version() == 1
    assert lib.io_png_band_rows() == png.UNFILTER_BAND
    mk = open(os.path.join(ROOT, "instaorder_amd", "csrc", "Makefile")).read()
    assert "png.hip" in mk and "png_inflate.h" in mk
    inf = open(os.path.join(ROOT, "instaorder_amd", "csrc", "png_inflate.h")).read()
    for s, text in png.STATUS.items():
        assert re.search(r"PNG_STATUS_\w+ = %d\b" % s, inf), s


def test_workspace_bytes_on_host_tables():
    ims = [c[0] for c in png_cases.batch_cases()[:6]]
    pool, desc = png.descriptors(ims, [0] * len(ims))
    assert pool.size == sum(len(im.deflate_bytes()) for im in ims)
    assert [d.data_off for d in desc] == list(np.cumsum([0] + [len(im.deflate_bytes()) for im in ims[:-1]]))
    assert [(d.H, d.W, d.channels, d.depth, d.adler) for d in desc] == [(im.H, im.W, im.channels, im.bit_depth, im.adler)
                                                                       for im in ims]
    header = (len(ims) + 1) * 8 + 15 & ~15
    assert png.workspace_bytes(desc) == header + sum((im.inflated_bytes + 15) // 16 * 16 for im in ims)
    for field, value in (("H", 0), ("W", 70000), ("channels", 2), ("depth", 4), ("data_bytes", -1), ("data_off", -1)):
        bad = (_lib.PngDesc * 1)()
        C.memmove(bad, C.byref(desc[0]), 48)
        setattr(bad[0], field, value)
        with pytest.raises(RuntimeError, match="refused"):
            png.workspace_bytes(bad)
    bad = (_lib.PngDesc * 1)()
    C.memmove(bad, C.byref(desc[0]), 48)
    bad[0].depth, bad[0].channels = 16, 3
    with pytest.raises(RuntimeError, match="1 of depth 16"):
        png.workspace_bytes(bad)


def test_inflate_under_the_sanitizers(tmp_path):
    """csrc/png_inflate.h compiled for the CPU with AddressSanitizer and UBSan: every intact image of the GPU tests, the
    three fuzz bases truncated and mutated, and the hand-made streams end clean; the status is 0 exactly for the streams
    Python's zlib accepts with the right byte count, it is the word ``inflate_walk`` states for every stream (so the exact
    word of each hand-made one), and the Adler-32 of the output is the one Python computes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "png_inflate_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "instaorder_amd", "csrc"),
                            os.path.join(ROOT, "tests", "png_inflate_host.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    ims = ([im for _, im in png_cases.damaged()] + [c[0] for c in png_cases.stream_cases()]
           + [c[0] for c in png_cases.batch_cases()])
    rec = str(tmp_path / "streams.bin")
    with open(rec, "wb") as f:
        f.write(png_cases.host_records(ims))
    run = subprocess.run([exe, rec], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    rows = [ln.split() for ln in run.stdout.splitlines()]
    assert len(rows) == len(ims)
    flagged = 0
    for (idx, status, adler), im in zip(rows, ims):
        status = int(status)
        want, raw = png.inflate_walk(im.deflate_bytes(), im.inflated_bytes)[:2]
        assert status == want, (im.name, status, want)
        d = zlib.decompressobj(-15)
        try:
            got = d.decompress(im.deflate_bytes())
            accepted = d.eof and len(got) == im.inflated_bytes
        except zlib.error:
            accepted = False
        assert (status == 0) == accepted, (im.name, status)
        if status == 0:
            assert int(adler) == zlib.adler32(raw) & 0xFFFFFFFF == zlib.adler32(got) & 0xFFFFFFFF, im.name
        flagged += status != 0
    assert len(rows) // 3 < flagged < len(rows)
    by_name = {im.name: int(r[1]) for r, im in zip(rows, ims)}
    for s in range(1, 8):
        assert by_name["status%d" % s] == s
    assert by_name["status8"] == 0 and by_name["status9"] == 0     # the checksum and the filter bytes are later stages
