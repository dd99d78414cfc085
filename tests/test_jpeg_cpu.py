"""Baseline JPEG files on the host: the parser, ``JpegImage.to_host()`` (the contract of the kernels) against what the
reference's ``Image.open(f).convert('RGB')`` made of the fixture files, the loader's fall-back, the ABI declarations, and
the entropy decoder the kernel compiles (csrc/jpeg_entropy.h) built for the CPU and run under the sanitizers on intact,
truncated and mutated streams.  All comparisons are exact; nothing here needs a GPU or Pillow (one test uses Pillow if it is
there)."""
import ctypes as C
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases
from helpers import ROOT
from instaorder_amd import _lib, jpeg

NAMES, CASES, UNSUPPORTED = jpeg_cases.load()


def _expect(name):
    m = re.match(r"(\d+)x(\d+)_(444|422|420|gray)_(q\d+|opt|rst\d+)$", name)
    H, W, form, tail = int(m.group(1)), int(m.group(2)), m.group(3), m.group(4)
    return H, W, form, tail


def test_parser_fields_of_every_case():
    assert len(NAMES) == len(set(NAMES)) >= 60
    for name in NAMES:
        data, rgb = CASES[name]
        im = jpeg.JpegImage(data, name=name)
        H, W, form, tail = _expect(name)
        assert im.supported and im.reason is None, (name, im.reason)
        assert im.shape == (H, W, 3) == rgb.shape and im.dtype == np.uint8
        assert im.nbytes_compressed == len(data)
        assert len(im.components) == (1 if form == "gray" else 3)
        assert im.luma_sampling == {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[form]
        assert im.restart_interval == (int(tail[3:]) if tail.startswith("rst") else 0)
        s, e = im.entropy
        assert data[e:e + 2] == b"\xff\xd9" and 0 < s < e and im.nbytes_entropy == e - s
        assert jpeg.is_jpeg(im) and not jpeg.is_jpeg(rgb)
        assert len(im.tables_blob()) == jpeg.TABLES_BYTES
        # the same through bytearray / memoryview, and with fill bytes in front of a marker and bytes after EOI
        if name == NAMES[3]:
            at = data.index(b"\xff\xdb")
            padded = data[:at] + b"\xff\xff" + data[at:] + b"trailing bytes"
            for d in (bytearray(data), memoryview(data), padded):
                assert np.array_equal(jpeg.JpegImage(d).to_host(), rgb)
    # files that were written with the same settings share their tables: one upload per batch
    blobs = {jpeg_cases.image(n).tables_blob() for n in NAMES if n.endswith("_444_q85")}
    assert len(blobs) == 1


def test_to_host_equals_the_reference_load_on_every_case():
    for name in NAMES:
        data, rgb = CASES[name]
        got = jpeg.JpegImage(data, name=name).to_host()
        assert got.dtype == np.uint8 and got.shape == rgb.shape, name
        assert np.array_equal(got, rgb), "%s: %d of %d bytes differ" % (name, (got != rgb).sum(), rgb.size)


def test_to_host_on_fresh_images():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(7)
    for H, W, kw in [(2, 3, dict(subsampling=1)), (3, 4, dict(subsampling=2)), (5, 2, dict(subsampling=2)),
                     (13, 29, dict(subsampling=2, quality=70)), (31, 18, dict(subsampling=1, quality=95)),
                     (24, 40, dict(subsampling=0, quality=50, optimize=True)),
                     (19, 50, dict(subsampling=2, quality=92, restart_marker_blocks=3))]:
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        bio = io.BytesIO()
        Image.fromarray(img).save(bio, "JPEG", **kw)
        ref = np.array(Image.open(io.BytesIO(bio.getvalue())).convert("RGB"))
        assert np.array_equal(jpeg.JpegImage(bio.getvalue()).to_host(), ref), (H, W, kw)


def test_unsupported_files_say_why():
    want = {"progressive": "progressive", "cmyk": "4 components", "440": "sampling 1x2"}
    assert set(UNSUPPORTED) == set(want)
    for kind, data in UNSUPPORTED.items():
        im = jpeg.JpegImage(data, name=kind)
        assert not im.supported and want[kind] in im.reason, (kind, im.reason)
        assert im.shape == (21, 35, 3)
        with pytest.raises(ValueError, match="not supported"):
            im.to_host()
    data = CASES["21x35_444_q85"][0]
    sof = data.index(b"\xff\xc0")

    def patched(at, value):
        b = bytearray(data)
        b[at] = value
        return bytes(b)

    for d, why in [(patched(sof + 4, 12), "12-bit"), (patched(sof + 6, 0), "zero dimension"),
                   (patched(sof + 1, 0xC9), "arithmetic"), (patched(sof + 12, 3), "quantisation table 3 is missing"),
                   (patched(sof + 10, ord("R")), "frame order")]:
        im = jpeg.JpegImage(d)
        assert not im.supported and why in im.reason, (why, im.reason)

    def rgb_ids(d):
        d = bytearray(d)
        f, c = bytes(d).index(b"\xff\xc0"), bytes(d).index(b"\xff\xda")
        d[f + 10], d[f + 13], d[f + 16] = b"RGB"
        d[c + 5], d[c + 7], d[c + 9] = b"RGB"
        return bytes(d)

    assert jpeg.JpegImage(rgb_ids(data)).supported           # a JFIF marker decides for YCbCr whatever the ids are
    # without the JFIF segment the ids R, G, B mean RGB; an Adobe segment with transform 1 means YCbCr again
    app0 = data.index(b"\xff\xe0")
    L = int.from_bytes(data[app0 + 2:app0 + 4], "big")
    bare = bytearray(data[:app0] + data[app0 + 2 + L:])
    assert jpeg.JpegImage(bytes(bare)).supported
    bare = rgb_ids(bare)
    im = jpeg.JpegImage(bare)
    assert not im.supported and "RGB" in im.reason
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01"
    assert jpeg.JpegImage(bare[:2] + adobe + bare[2:]).supported
    assert "RGB" in jpeg.JpegImage(bare[:2] + adobe[:-1] + b"\x00" + bare[2:]).reason
    # a second scan
    eoi = data.rindex(b"\xff\xd9")
    sos = data.index(b"\xff\xda")
    two = data[:eoi] + data[sos:]
    im = jpeg.JpegImage(two)
    assert not im.supported and "2 scans" in im.reason


def test_broken_marker_structure_raises():
    data = CASES["9x17_420_q85"][0]
    sos = data.index(b"\xff\xda")
    for bad in (b"", b"\xff\xd8", b"\x89PNG" + data, data[:10], data[:sos + 4], data[:-2],
                data[:2] + b"\x00" + data[2:], data[:2] + b"\xff\xe1\xff\xff" + data[2:],
                data[:2] + data[sos:], data[:2] + b"\xff\xd8" + data[2:]):
        with pytest.raises(ValueError):
            jpeg.JpegImage(bad)


def test_damaged_streams_are_flagged_not_decoded():
    im = jpeg_cases.image("21x35_444_rst2")
    ent = im.entropy_bytes()
    assert jpeg_cases.status_of(im)[0] == 0
    assert jpeg_cases.status_of(im.with_entropy(ent[:len(ent) // 2]))[0] in (3, 4)
    first = ent.index(b"\xff\xd0")
    swapped = ent[:first] + b"\xff\xd1" + ent[first + 2:]
    assert jpeg_cases.status_of(im.with_entropy(swapped))[0] == 3
    with pytest.raises(jpeg.JpegStreamError, match="restart"):
        im.with_entropy(swapped).to_host()


def test_loader_returns_jpeg_or_falls_back(tmp_path):
    ok, rgb = CASES["16x16_420_q85"]
    (tmp_path / "a.jpg").write_bytes(ok)
    (tmp_path / "p.jpg").write_bytes(UNSUPPORTED["progressive"])
    (tmp_path / "n.bin").write_bytes(b"not a jpeg at all")
    seen = []

    def fallback(path):
        seen.append(os.path.basename(path))
        return np.zeros((21, 35, 3), np.uint8)

    load = jpeg.loader(str(tmp_path), fallback=fallback)
    a = load("a.jpg")
    assert jpeg.is_jpeg(a) and a.supported and a.name == "a.jpg" and np.array_equal(a.to_host(), rgb) and not seen
    assert load("p.jpg").shape == (21, 35, 3) and load("n.bin").dtype == np.uint8
    assert seen == ["p.jpg", "n.bin"]
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="Pillow"):
            jpeg.loader(str(tmp_path))("p.jpg")
    else:
        got = jpeg.loader(str(tmp_path))("p.jpg")
        assert isinstance(got, np.ndarray) and got.shape == (21, 35, 3) and got.dtype == np.uint8


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    for name, nargs in (("io_jpeg_decode_u8", 14), ("io_jpeg_workspace_bytes", 2)):
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name + " is not declared in include/instaorder_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    assert "} io_jpeg_desc;" in hdr and "} io_jpeg_tables;" in hdr
    assert C.sizeof(_lib.JpegDesc) == 64 and jpeg.TABLES_BYTES == 512 + 64 + 1024
    lib = _lib.lib()
    assert hasattr(lib, "io_jpeg_decode_u8") and hasattr(lib, "io_jpeg_workspace_bytes")
    assert lib.io_abi_version() == 1
    ent = open(os.path.join(ROOT, "instaorder_amd", "csrc", "jpeg_entropy.h")).read()
    assert int(ent.split("#define JPEG_LOOKUP_BITS")[1].split()[0]) == jpeg.LOOKUP_BITS
    assert lib.io_jpeg_lds_table_sets() == int(hdr.split("#define IO_JPEG_LDS_TABLE_SETS")[1].split()[0])
    assert "jpeg.hip" in open(os.path.join(ROOT, "instaorder_amd", "csrc", "Makefile")).read()


def test_workspace_bytes_on_host_tables():
    ims = [jpeg_cases.image(n) for n in ("9x17_420_q85", "21x35_422_q85", "33x47_444_q85", "40x24_gray_q85", "1x1_420_q85")]
    pool, tables, desc = jpeg.descriptors(ims, [0] * len(ims))
    assert tables.size == 2 * jpeg.TABLES_BYTES                 # colour files share one set, the grayscale file has its own
    assert pool.size == sum(im.nbytes_entropy for im in ims) and [d.data_off for d in desc] == list(
        np.cumsum([0] + [im.nbytes_entropy for im in ims[:-1]]))
    # 8 x 8 blocks: 4:2:0 9x17 -> 1 x 2 MCUs of 6; 4:2:2 21x35 -> 3 x 3 of 4; 4:4:4 33x47 -> 5 x 6 of 3; gray 40x24 -> 15; 1x1 -> 6
    blocks = 12 + 36 + 90 + 15 + 6
    header = (len(ims) + 1) * 8 + 15 & ~15
    assert jpeg.workspace_bytes(desc) == header + 2 * 4 * 904 + blocks * (128 + 64)
    for field, value in (("hs", 3), ("n_comp", 2), ("H", 0), ("W", 70000), ("restart_interval", -1), ("table_set", -1)):
        bad = (_lib.JpegDesc * 1)()
        C.memmove(bad, C.byref(desc[0]), 64)
        setattr(bad[0], field, value)
        with pytest.raises(RuntimeError, match="refused"):
            jpeg.workspace_bytes(bad)
    bad = (_lib.JpegDesc * 1)()
    C.memmove(bad, C.byref(desc[0]), 64)
    bad[0].dc[1] = 2
    with pytest.raises(RuntimeError, match="Huffman < 2"):
        jpeg.workspace_bytes(bad)


def test_entropy_decoder_under_the_sanitizers(tmp_path):
    """csrc/jpeg_entropy.h compiled for the CPU with AddressSanitizer and UBSan: three fixture streams as they are, truncated
    at every byte and with 1000 mutations each end clean, every run decoded or flagged; the statuses (and the coefficients
    of the runs that decode) are what ``JpegImage.coefficients`` says for a sample of them."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_entropy_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "instaorder_amd", "csrc"),
                            os.path.join(ROOT, "tests", "jpeg_entropy_host.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    ims = [jpeg_cases.image(n) for n in jpeg_cases.FUZZ]
    files = []
    for k, im in enumerate(ims):
        files.append(str(tmp_path / ("stream%d.bin" % k)))
        with open(files[-1], "wb") as f:
            f.write(jpeg_cases.stream_file(im))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    rows = [ln.split() for ln in run.stdout.splitlines()]
    assert len(rows) == sum(1 + im.nbytes_entropy + 1000 for im in ims)
    assert all(0 <= int(r[3]) <= 5 for r in rows)
    flagged = sum(int(r[3]) != 0 for r in rows)
    assert flagged > len(rows) // 2 and flagged < len(rows)      # most damage is caught, some mutations still decode
    # the Python statement of the decoder agrees: every intact stream, every 7th truncation (and the two that
    # tests/test_gpu_jpeg.py uses), the first 60 mutations
    for s, kind, idx, status, checksum in rows:
        s, idx, status = int(s), int(idx), int(status)
        ent = ims[s].entropy_bytes()
        if kind == "I":
            alt = ims[s]
        elif kind == "T" and (idx % 7 == 0 or idx in (len(ent) // 3, len(ent) - 1)):
            alt = ims[s].with_entropy(ent[:idx])
        elif kind == "M" and idx < 60:
            alt = ims[s].with_entropy(jpeg_cases.mutated(ent, idx))
        else:
            continue
        want, csum = jpeg_cases.status_of(alt)
        assert status == want, (jpeg_cases.FUZZ[s], kind, idx, status, want)
        if want == 0:
            assert int(checksum) == csum, (jpeg_cases.FUZZ[s], kind, idx)
