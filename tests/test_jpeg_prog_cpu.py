"""Progressive JPEG files on the host: the parser (scans, their tables, restart intervals and levels), ``to_host()`` (the
contract of the kernels) against what the reference's ``Image.open(f).convert('RGB')`` made of the fixture files, the opt-in
surface, the refusals, the ABI declarations, and the scan decoder the kernel compiles (csrc/jpeg_prog.h) built for the CPU
and run under the sanitizers on intact, truncated and mutated scans.  All comparisons are exact; nothing here needs a GPU or
Pillow."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import jpeg_cases
import jpeg_prog_cases as cases
from helpers import ROOT
from instaorder_amd import _lib, jpeg, png

NAMES, CASES, UNSUPPORTED = cases.load()


def _form(name):
    m = re.match(r"(\d+)x(\d+)_(444|422|420|gray)_(\w+)$", name)
    return int(m.group(1)), int(m.group(2)), m.group(3), m.group(4)


def test_parser_scans_tables_and_levels():
    assert len(NAMES) == len(set(NAMES)) >= 40
    for name in NAMES:
        data, rgb = CASES[name]
        im = cases.image(name)
        H, W, form, tail = _form(name)
        assert im.supported and im.progressive and im.reason is None, (name, im.reason)
        assert im.shape == (H, W, 3) == rgb.shape and jpeg.is_jpeg(im)
        assert im.luma_sampling == {"444": (1, 1), "422": (2, 1), "420": (2, 2), "gray": (1, 1)}[form]
        nc = len(im.components)
        assert nc == (1 if form == "gray" else 3)
        levels = im.scan_levels()
        if form == "gray":                                       # Pillow's scripts: 6 scans for one component, 10 for three
            assert len(im.scans) == 6 and max(levels) + 1 == 4, (name, levels)
        else:
            assert len(im.scans) == 10 and max(levels) + 1 == 4, (name, levels)
        ri = int(tail[3:]) if tail.startswith("rst") else 0
        seen, at = {}, 0
        for n, (sc, lv) in enumerate(zip(im.scans, levels)):
            assert sc.restart_interval == ri and at < sc.start < sc.end and data[sc.end] == 0xFF, (name, n)
            at = sc.end
            assert len(sc.comps) in (1, nc) and list(sc.comps) == sorted(sc.comps) and len(sc.tables) == len(sc.comps)
            assert (sc.ss == 0 and sc.se == 0) or (len(sc.comps) == 1 and 1 <= sc.ss <= sc.se <= 63)
            for t in sc.tables:                                  # a DC refinement reads plain bits, every other scan a table
                assert (t is None) == (sc.ss == 0 and sc.ah > 0)
                assert t is None or (len(t[0]) == 16 and sum(t[0]) == len(t[1]) > 0)
            # the level rule the library checks: strictly above every earlier scan that shares a coefficient
            for c in sc.comps:
                for k in range(sc.ss, sc.se + 1):
                    assert lv > seen.get((c, k), -1), (name, n)
                    seen[(c, k)] = lv
            assert im.scan_bytes(n) == data[sc.start:sc.end]
        assert levels[0] == 0 and im.scans[0].ss == 0
        assert data[im.scans[-1].end:im.scans[-1].end + 2] == b"\xff\xd9"
    # Pillow writes a DHT in front of almost every scan, reusing the table ids: the scans of one file carry different tables
    im = cases.image("33x47_420_q85")
    ac = [sc.tables[0] for sc in im.scans if sc.ss > 0]
    assert len(set(ac)) > 4
    assert [lv for lv in im.scan_levels()] == [0, 1, 1, 1, 1, 2, 1, 2, 2, 3]
    assert cases.image("33x47_420_swapped").scan_levels() == [0, 1, 1, 1, 1, 2, 1, 2, 2, 3]
    assert cases.image("33x47_420_lumafirst").scan_levels() == [0, 1, 1, 2, 3, 1, 1, 1, 2, 2]
    assert [sc.comps for sc in cases.image("33x47_420_swapped").scans[2:4]] == [(1,), (2,)]
    assert [sc.comps for sc in im.scans[2:4]] == [(2,), (1,)]
    # a one-component luma scan walks its own raster: 21x35 at 4:2:0 is 5 x 3 blocks against the 6 x 4 of the MCU grid
    im = cases.image("21x35_420_q85")
    order, per_mcu, bw, bh = im.scan_blocks(1)
    assert im.scans[1].comps == (0,) and (bw, bh, per_mcu) == (5, 3, 1) and len(order) == 15
    assert list(order[:6]) == [0, 1, 6, 7, 12, 2] and im.scan_blocks(0)[1:] == (6, 3, 2)


def test_to_host_equals_the_reference_load_on_every_case():
    for name in NAMES:
        data, rgb = CASES[name]
        got = cases.image(name).to_host()
        assert got.dtype == np.uint8 and got.shape == rgb.shape, name
        assert np.array_equal(got, rgb), "%s: %d of %d bytes differ" % (name, (got != rgb).sum(), rgb.size)


def test_the_fixture_covers_the_hard_paths():
    tot = dict(eobrun_max=0, eobrun_refine_max=0, zrl_refine=0, correction_bits=0, restarts=0)
    for name in ("96x136_420_q20", "33x47_444_q100", "33x47_444_rst1"):
        st = {}
        im = cases.image(name)
        coef = im.coefficients(st)
        assert coef.dtype == np.int16 and coef.shape[1] == 64
        for k in tot:
            tot[k] = max(tot[k], st[k])
    mw = -(-136 // 16)
    assert tot["eobrun_max"] > 2 * mw and tot["eobrun_refine_max"] > 1 and tot["zrl_refine"] > 0
    assert tot["correction_bits"] > 1000 and tot["restarts"] > 0


def test_opt_in_surface(tmp_path):
    assert jpeg.get_progressive() == "host"
    for name in NAMES:
        im = jpeg.JpegImage(CASES[name][0], name=name)
        assert not im.supported and not im.progressive and "progressive" in im.reason, (name, im.reason)
        with pytest.raises(ValueError, match="not supported"):
            im.to_host()
    name = "16x16_420_q85"
    (tmp_path / "p.jpg").write_bytes(CASES[name][0])
    (tmp_path / "b.jpg").write_bytes(jpeg_cases.load()[1][name][0])
    seen = []

    def fallback(path):
        seen.append(os.path.basename(path))
        return np.zeros((16, 16, 3), np.uint8)

    assert isinstance(jpeg.loader(str(tmp_path), fallback=fallback)("p.jpg"), np.ndarray) and seen == ["p.jpg"]
    got = jpeg.loader(str(tmp_path), fallback=fallback, progressive=True)("p.jpg")
    assert jpeg.is_jpeg(got) and got.progressive and np.array_equal(got.to_host(), CASES[name][1]) and seen == ["p.jpg"]
    got = png.loader(str(tmp_path), fallback=fallback, jpeg=True, progressive=True)("p.jpg")
    assert jpeg.is_jpeg(got) and got.progressive and seen == ["p.jpg"]
    base = jpeg.loader(str(tmp_path), fallback=fallback, progressive=True)("b.jpg")
    assert jpeg.is_jpeg(base) and not base.progressive and base.supported
    try:                                                         # the module setting is read when a file is loaded
        jpeg.set_progressive("device")
        assert jpeg.get_progressive() == "device"
        assert jpeg.JpegImage(CASES[name][0]).progressive
        assert jpeg.loader(str(tmp_path), fallback=fallback)("p.jpg").progressive
        assert not jpeg.JpegImage(CASES[name][0], progressive=False).supported
    finally:
        jpeg.set_progressive("host")
    assert not jpeg.JpegImage(CASES[name][0]).supported
    with pytest.raises(ValueError, match="'host' or 'device'"):
        jpeg.set_progressive("gpu")
    assert jpeg.get_progressive() == "host"
    # the environment variable, read at import: in a fresh interpreter
    code = "from instaorder_amd import jpeg; print(jpeg.get_progressive())"
    for value, want in (("device", "device"), ("", "host")):
        env = dict(os.environ, IO_JPEG_PROGRESSIVE=value, PYTHONPATH=ROOT)
        run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert run.returncode == 0 and run.stdout.split()[-1] == want, run.stderr[-2000:]
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                         env=dict(os.environ, IO_JPEG_PROGRESSIVE="devcie", PYTHONPATH=ROOT))
    assert run.returncode != 0 and "set_progressive" in run.stderr and "devcie" in run.stderr


def test_refused_files_name_their_reason():
    want = {"incomplete": "incomplete progression", "acfirst": "in front of the DC scan", "quant16": "16-bit quantisation table"}
    assert set(UNSUPPORTED) == set(want)
    for kind, data in UNSUPPORTED.items():
        im = jpeg.JpegImage(data, name=kind, progressive=True)
        assert not im.supported and not im.progressive and want[kind] in im.reason and "progressive" in im.reason, (kind, im.reason)
        assert im.shape == (33, 47, 3)
        with pytest.raises(ValueError, match="not supported"):
            im.to_host()
    data = CASES["33x47_420_q85"][0]
    sos = [m.start() for m in re.finditer(b"\xff\xda\x00[\x08\x0c]", data)]
    assert len(sos) == 10

    def patched(at, value):
        b = bytearray(data)
        b[at] = value
        return bytes(b)

    # the SOS of scan 1 (luma 1..5, Al 2): FF DA, length 8, 1 component, id, tables, Ss, Se, AhAl
    s1 = sos[1]
    assert data[s1 + 4] == 1 and data[s1 + 7:s1 + 10] == b"\x01\x05\x02"
    sof = data.index(b"\xff\xc2")
    for d, why in [(patched(s1 + 7, 0), "mixes DC and AC"), (patched(s1 + 9, 0x0e), "Al 14 above 13"),
                   (patched(s1 + 9, 0x42), "refines by more than one bit"), (patched(s1 + 9, 0x21), "not at Al 2"),
                   (patched(s1 + 8, 9), "a second time"), (patched(s1 + 5, 77), "components of the frame"),
                   (patched(s1 + 6, 0x03), "Huffman table that is missing"), (patched(sof + 4, 12), "12-bit"),
                   (patched(sof + 11, 0x12), "sampling 1x2")]:
        im = jpeg.JpegImage(d, progressive=True)
        assert not im.supported and why in im.reason, (why, im.reason)
    # a quantisation table between two scans
    dqt = data.index(b"\xff\xdb")
    L = int.from_bytes(data[dqt + 2:dqt + 4], "big")
    late = data[:sos[3]] + data[dqt:dqt + 2 + L] + data[sos[3]:]
    im = jpeg.JpegImage(late, progressive=True)
    assert not im.supported and "between scans" in im.reason
    # a DC scan of two of the three components
    s0 = sos[0]
    assert data[s0 + 4] == 3
    two = data[:s0 + 2] + b"\x00\x0a\x02" + data[s0 + 5:s0 + 9] + data[s0 + 11:]
    im = jpeg.JpegImage(two, progressive=True)
    assert not im.supported and "2 of 3 components" in im.reason


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    for name, nargs in (("io_jpeg_decode_prog_u8", 23), ("io_jpeg_prog_workspace_bytes", 4)):
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name + " is not declared in include/instaorder_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    for struct in ("io_jpeg_prog_scan", "io_jpeg_prog_image", "io_jpeg_huff_raw"):
        assert "} %s;" % struct in hdr
    assert C.sizeof(_lib.JpegProgScan) == 64 and C.sizeof(_lib.JpegProgImage) == 16 and C.sizeof(_lib.JpegHuffRaw) == 272
    lib = _lib.lib()
    assert hasattr(lib, "io_jpeg_decode_prog_u8") and hasattr(lib, "io_jpeg_prog_workspace_bytes")
    assert lib.io_abi_version() == 1
    mk = open(os.path.join(ROOT, "instaorder_amd", "csrc", "Makefile")).read()
    assert "jpeg_prog.h" in mk
    assert "IO_PROF_JPEG_PROG_ENTROPY" in open(os.path.join(ROOT, "instaorder_amd", "csrc", "io_common.h")).read()
    assert '"jpeg_prog_entropy"' in open(os.path.join(ROOT, "instaorder_amd", "csrc", "capi.hip")).read()


def test_descriptors_and_workspace_bytes_on_host_tables():
    ims = [cases.image(n) for n in ("9x17_422_q85", "21x35_420_q85", "33x47_444_q85", "40x24_gray_q85", "1x1_420_q85",
                                     "21x35_420_q85")]
    p = jpeg.descriptors_progressive(ims, [0] * len(ims))
    assert p["n_scans"] == 5 * 10 + 6 and [r.first_scan for r in p["image"]] == [0, 10, 20, 30, 36, 46]
    assert [r.n_levels for r in p["image"]] == [4] * 6
    assert p["tables"].size == 2 * jpeg.TABLES_BYTES            # colour files share their quantisation set, gray has its own
    # identical Huffman tables are stored once: the repeated image adds none
    q = jpeg.descriptors_progressive(ims[:5], [0] * 5)
    assert p["huff"].size == q["huff"].size and p["huff"].size % 272 == 0
    assert p["pool"].size == sum(cases.total_scan_bytes(im) for im in ims)
    sc = p["scan"][11]
    assert (sc.image, sc.n_comp, sc.comp[0], sc.ss, sc.se, sc.ah, sc.al, sc.level) == (1, 1, 0, 1, 5, 0, 2, 1)
    blocks = 16 + 36 + 90 + 15 + 6 + 36                          # 9x17 4:2:2 -> 2 x 2 MCUs of 4; 21x35 4:2:0 -> 3 x 2 of 6; ...
    header = (len(ims) + 1) * 8 + 15 & ~15
    n_huff = p["huff"].size // 272
    assert jpeg.workspace_bytes_progressive(p) == header + (n_huff * 904 + 15 & ~15) + blocks * (128 + 64) + (56 * 4 + 15 & ~15)
    lib = _lib.lib()
    assert lib.io_jpeg_prog_workspace_bytes(C.cast(p["desc"], C.c_void_p), len(ims), 0, 56) == 0
    assert lib.io_jpeg_prog_workspace_bytes(C.cast(p["desc"], C.c_void_p), len(ims), n_huff, 0) == 0
    with pytest.raises(ValueError, match="baseline"):
        jpeg.descriptors_progressive([jpeg_cases.image("9x17_420_q85")], [0])


def test_scan_decoder_under_the_sanitizers(tmp_path):
    """csrc/jpeg_prog.h compiled for the CPU with AddressSanitizer and UBSan: every fixture as it is, with each scan truncated
    (at every byte; every 16th on the large file) and with 64 mutations per scan ends clean, every run decoded or flagged;
    the intact runs give the coefficients of ``JpegImage.coefficients``."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_prog_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "instaorder_amd", "csrc"),
                            os.path.join(ROOT, "tests", "jpeg_prog_host.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    ims = [cases.image(n) for n in NAMES]
    files = []
    for k, im in enumerate(ims):
        files.append(str(tmp_path / ("image%d.bin" % k)))
        with open(files[-1], "wb") as f:
            f.write(cases.image_file(im))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    rows = [ln.split() for ln in run.stdout.splitlines()]
    want_rows = 0
    for im in ims:
        step = cases.STRIDE if cases.total_scan_bytes(im) > cases.EVERY_BYTE else 1
        want_rows += 1 + sum(len(range(0, len(im.scan_bytes(n)), step)) + cases.MUTATIONS for n in range(len(im.scans)))
    assert len(rows) == want_rows
    assert all(0 <= int(r[4]) <= 5 for r in rows)
    assert {int(r[4]) for r in rows} == {0, 1, 2, 3, 4}          # a DC category above 15 needs a table that has such a symbol
    assert all(int(r[4]) != 0 for r in rows if r[1] == "T")      # a truncated scan never decodes
    intact = [r for r in rows if r[1] == "I"]
    assert len(intact) == len(ims)
    for r in intact:
        assert int(r[4]) == 0 and int(r[5]) == cases.checksum(ims[int(r[0])].coefficients()), NAMES[int(r[0])]
    # the Python statement of the decoder agrees on the status of a sample of the damaged scans, and on the coefficients
    # of the mutations that still decode
    k = NAMES.index("21x35_420_rst2")
    checked = 0
    for r in rows:
        if int(r[0]) != k or r[1] != "M" or int(r[3]) >= 16:
            continue
        n, m = int(r[2]), int(r[3])
        alt = ims[k].with_scan(n, cases.mutated(ims[k].scan_bytes(n), m))
        try:
            got = (0, cases.checksum(alt.coefficients()))
        except jpeg.JpegStreamError as e:
            got = (e.status, None)
        assert got[0] == int(r[4]), (n, m, got, r)
        if got[0] == 0:
            assert got[1] == int(r[5]), (n, m)
        checked += 1
    assert checked == 160
