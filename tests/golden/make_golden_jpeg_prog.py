"""Writes tests/golden/jpeg_prog_cases.npz: small progressive JPEG files and what the reference's own image load
(``np.array(Image.open(f).convert('RGB'))``, datasets/occ_order_dataset.py:66-79) makes of them, so that the tests need no
Pillow.  Needs Pillow (with libjpeg-turbo or libjpeg 6b and later: the default decoder settings) and NumPy:

    python tests/golden/make_golden_jpeg_prog.py

Besides Pillow's own files there are two whose scan units (the DHT segments, the SOS and its data) were put into another
order -- Cr before Cb, and luma finished before chroma -- which Pillow decodes for the expected arrays, and three files the
device must refuse.  The script asserts what the set covers and that ``JpegImage.to_host()`` equals Pillow on every case.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from instaorder_amd import jpeg  # noqa: E402
from make_golden_jpeg import SAMPLING, SIZES, picture  # noqa: E402


def encode(img, form, **kw):
    bio = io.BytesIO()
    if form == "gray":
        Image.fromarray(img[:, :, 0]).save(bio, "JPEG", progressive=True, **kw)
    else:
        Image.fromarray(img).save(bio, "JPEG", progressive=True, subsampling=SAMPLING[form], **kw)
    return bio.getvalue()


def smooth(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([120 + 100 * np.sin(x / 40. + y / 70.), 128 + 90 * np.cos(y / 55.), (x + 2 * y) * 0.6], 2).clip(
        0, 255).astype(np.uint8)


def split_scans(data):
    """(head, [scan unit], tail): a scan unit is the DHT / DRI segments in front of an SOS, the SOS and its data"""
    p, n = 2, len(data)
    head_end, units, unit_start = None, [], None
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == 0xD9:
            break
        L = int.from_bytes(data[p + 2:p + 4], "big")
        p += 2 + L
        if m == 0xC2:                                            # Pillow writes every DHT behind the frame header
            head_end = unit_start = p
        elif m == 0xDA:
            assert head_end is not None
            while not (data[p] == 0xFF and data[p + 1] != 0 and not 0xD0 <= data[p + 1] <= 0xD7):
                p += 1
            units.append(data[unit_start:p])
            unit_start = p
        else:
            assert m in (0xC4, 0xDD) or head_end is None, "segment 0x%02x between scans" % m
    assert p + 2 == n and unit_start == p
    return data[:head_end], units, data[p:]


def main():
    rng = np.random.RandomState(20261019)
    pics = {hw: picture(hw[0], hw[1], rng) for hw in SIZES + [(160, 208)]}      # the pictures of make_golden_jpeg.py
    cases = []
    for (H, W) in SIZES:
        for form in ("444", "422", "420", "gray"):
            cases.append(("%dx%d_%s_q85" % (H, W, form), encode(pics[(H, W)], form, quality=85)))
    for (H, W), form in [((1, 1), "420"), ((9, 17), "422"), ((21, 35), "420"), ((33, 47), "444"), ((33, 47), "gray")]:
        for q in (30, 100):
            cases.append(("%dx%d_%s_q%d" % (H, W, form, q), encode(pics[(H, W)], form, quality=q)))
    # restart intervals that do not divide the MCUs of a row (33x47: 6 / 3 per row, 21x35: 5 / 3, 40x24: 3 / 2)
    for (H, W), form, ri in [((33, 47), "444", 1), ((21, 35), "420", 2), ((21, 35), "444", 3), ((33, 47), "422", 2),
                             ((40, 24), "gray", 2), ((9, 17), "420", 1)]:
        cases.append(("%dx%d_%s_rst%d" % (H, W, form, ri), encode(pics[(H, W)], form, quality=85, restart_marker_blocks=ri)))
    cases.append(("96x136_420_q20", encode(smooth(96, 136), "420", quality=20)))
    head, units, tail = split_scans(encode(pics[(33, 47)], "420", quality=85))
    assert len(units) == 10
    # Pillow's colour script: 0 DC, 1 Y 1-5, 2 Cr, 3 Cb, 4 Y 6-63, 5 Y refine, 6 DC refine, 7 Cr refine, 8 Cb refine, 9 Y refine
    cases.append(("33x47_420_swapped", head + b"".join(units[k] for k in (0, 1, 3, 2, 4, 5, 6, 8, 7, 9)) + tail))
    cases.append(("33x47_420_lumafirst", head + b"".join(units[k] for k in (0, 1, 4, 5, 9, 6, 2, 3, 7, 8)) + tail))

    out = {"names": np.array([c[0] for c in cases])}
    cover = dict(eobrun=0, eobrun_row=0, eobrun_refine=0, zrl_refine=0, correction=0, restart=0, narrow=0, one=0)
    total = dict(eobrun_max=0, eobrun_refine_max=0, zrl_refine=0, correction_bits=0)
    for k, (name, b) in enumerate(cases):
        ref = np.array(Image.open(io.BytesIO(b)).convert("RGB"))
        im = jpeg.JpegImage(b, name=name, progressive=True)
        assert im.supported and im.progressive, (name, im.reason)
        assert not jpeg.JpegImage(b).supported
        st = {}
        im.coefficients(st)
        got = im.to_host()
        assert np.array_equal(got, ref), "%s: %d of %d bytes differ" % (name, (got != ref).sum(), ref.size)
        hs, vs = im.luma_sampling
        mw, mh = -(-im.W // (8 * hs)), -(-im.H // (8 * vs))
        cover["eobrun"] += st["eobrun_max"] > 1
        cover["eobrun_row"] += st["eobrun_max"] > mw * hs
        cover["eobrun_refine"] += st["eobrun_refine_max"] > 1
        cover["zrl_refine"] += st["zrl_refine"] > 0
        cover["correction"] += st["correction_bits"] > 0
        cover["restart"] += st["restarts"] > 0 and any(b"\xff\xd0" in im.scan_bytes(n) for n in range(len(im.scans)))
        for n, sc in enumerate(im.scans):
            _, _, bw, bh = im.scan_blocks(n)
            cover["narrow"] += sc.comps == (0,) and len(im.components) == 3 and bw < mw * hs and bh < mh * vs
        cover["one"] += (im.H, im.W) == (1, 1)
        total["eobrun_max"] = max(total["eobrun_max"], st["eobrun_max"])
        total["eobrun_refine_max"] = max(total["eobrun_refine_max"], st["eobrun_refine_max"])
        total["zrl_refine"] += st["zrl_refine"]
        total["correction_bits"] += st["correction_bits"]
        out["file_%d" % k] = np.frombuffer(b, np.uint8)
        out["rgb_%d" % k] = ref
    assert all(v > 0 for v in cover.values()), cover
    im = jpeg.JpegImage(dict(cases)["21x35_420_q85"], progressive=True)
    assert [im.scan_blocks(n)[2:] for n, sc in enumerate(im.scans) if sc.comps == (0,)][0] == (5, 3)
    print("coverage (cases with the property):", cover)
    print("over all cases:", total)

    units_ = list(units)
    out["unsupported_incomplete"] = np.frombuffer(head + b"".join(units_[:9]) + tail, np.uint8)
    out["unsupported_acfirst"] = np.frombuffer(head + b"".join(units_[k] for k in (1, 0, 2, 3, 4, 5, 6, 7, 8, 9)) + tail, np.uint8)
    b = dict(cases)["33x47_420_q85"]                             # a hand-built 16-bit DQT: every entry widened to two bytes
    at = b.index(b"\xff\xdb")
    L = int.from_bytes(b[at + 2:at + 4], "big")
    seg, wide, i = b[at + 4:at + 2 + L], b"", 0
    while i < len(seg):
        wide += bytes([0x10 | seg[i]]) + b"".join(bytes([0, v]) for v in seg[i + 1:i + 65])
        i += 65
    out["unsupported_quant16"] = np.frombuffer(b[:at] + b"\xff\xdb" + (len(wide) + 2).to_bytes(2, "big") + wide + b[at + 2 + L:],
                                               np.uint8)
    for key, why in (("incomplete", "incomplete progression"), ("acfirst", "in front of the DC scan"),
                     ("quant16", "16-bit quantisation table")):
        im = jpeg.JpegImage(out["unsupported_" + key].tobytes(), progressive=True)
        assert not im.supported and why in im.reason, (key, im.reason)
        print("unsupported %-12s %s" % (key, im.reason))

    path = os.path.join(HERE, "jpeg_prog_cases.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d bytes -> %s" % (len(cases), os.path.getsize(path), path))


if __name__ == "__main__":
    main()
