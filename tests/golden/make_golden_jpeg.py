"""Writes tests/golden/jpeg_cases.npz: small JPEG files and what the reference's own image load
(``np.array(Image.open(f).convert('RGB'))``, datasets/occ_order_dataset.py:66-79) makes of them, so that the tests need no
Pillow.  Needs Pillow (with libjpeg-turbo or libjpeg 6b and later: the default decoder settings) and NumPy:

    python tests/golden/make_golden_jpeg.py

The cases are the smallest shapes at which each stage can still go wrong; the script asserts what the set covers.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from instaorder_amd import jpeg  # noqa: E402

SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (21, 35), (33, 47), (40, 24)]
SAMPLING = {"444": 0, "422": 1, "420": 2}


def picture(H, W, rng):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([127 + 90 * np.sin(x / 5. + y / 9.) + rng.randn(H, W) * 25,
                     127 + 90 * np.cos(y / 4.) + rng.randn(H, W) * 25,
                     (x * y * 3.) % 256 + rng.randn(H, W) * 10], 2).clip(0, 255).astype(np.uint8)


def encode(img, form, **kw):
    bio = io.BytesIO()
    if form == "gray":
        Image.fromarray(img[:, :, 0]).save(bio, "JPEG", **kw)
    else:
        Image.fromarray(img).save(bio, "JPEG", subsampling=SAMPLING[form], **kw)
    return bio.getvalue()


def main():
    rng = np.random.RandomState(20261019)
    cases = []                                               # (name, bytes)
    pics = {hw: picture(hw[0], hw[1], rng) for hw in SIZES + [(160, 208)]}
    for (H, W) in SIZES:
        for form in ("444", "422", "420", "gray"):
            cases.append(("%dx%d_%s_q85" % (H, W, form), encode(pics[(H, W)], form, quality=85)))
    for (H, W) in [(1, 1), (9, 17), (21, 35), (33, 47)]:
        for form in ("444", "422", "420", "gray"):
            for q in (30, 100):
                cases.append(("%dx%d_%s_q%d" % (H, W, form, q), encode(pics[(H, W)], form, quality=q)))
    for (H, W), form in [((9, 17), "444"), ((21, 35), "420"), ((33, 47), "422"), ((40, 24), "gray")]:
        cases.append(("%dx%d_%s_opt" % (H, W, form), encode(pics[(H, W)], form, quality=85, optimize=True)))
    # restart intervals that do not divide the MCUs of a row: 33x47 has 6 (4:4:4), 3 (4:2:2, 4:2:0) MCUs per row, 21x35 5 / 3
    for (H, W), form, ri in [((33, 47), "444", 1), ((21, 35), "444", 2), ((21, 35), "444", 3), ((33, 47), "420", 2),
                             ((21, 35), "422", 2), ((33, 47), "gray", 1), ((9, 17), "420", 1), ((40, 24), "444", 2),
                             ((21, 35), "gray", 3)]:
        cases.append(("%dx%d_%s_rst%d" % (H, W, form, ri), encode(pics[(H, W)], form, quality=85, restart_marker_blocks=ri)))
    cases.append(("160x208_420_q90", encode(pics[(160, 208)], "420", quality=90)))

    out = {"names": np.array([c[0] for c in cases])}
    cover = dict(zrl=0, long_code=0, dc8=0, odd_chroma=0, restart=0)
    for k, (name, b) in enumerate(cases):
        ref = np.array(Image.open(io.BytesIO(b)).convert("RGB"))
        im = jpeg.JpegImage(b, name=name)
        assert im.supported, (name, im.reason)
        st = {}
        im.coefficients(st)
        hs, vs = im.luma_sampling
        cover["zrl"] += st["zrl"] > 0
        cover["long_code"] += st["max_code_length"] > jpeg.LOOKUP_BITS
        cover["dc8"] += st["max_dc_category"] >= 8
        cover["odd_chroma"] += (hs, vs) == (2, 2) and (-(-im.W // 2)) % 2 == 1 and (-(-im.H // 2)) % 2 == 1
        cover["restart"] += im.restart_interval > 0 and b"\xff\xd0" in im.entropy_bytes()
        if im.restart_interval:
            mw = -(-im.W // (8 * hs))
            assert mw % im.restart_interval or im.restart_interval == 1, name
        out["file_%d" % k] = np.frombuffer(b, np.uint8)
        out["rgb_%d" % k] = ref
    assert all(v > 0 for v in cover.values()), cover
    print("coverage (cases with the property):", cover)

    pic = pics[(21, 35)]
    bio = io.BytesIO()
    Image.fromarray(pic).save(bio, "JPEG", quality=85, progressive=True)
    out["unsupported_progressive"] = np.frombuffer(bio.getvalue(), np.uint8)
    bio = io.BytesIO()
    Image.fromarray(pic).convert("CMYK").save(bio, "JPEG", quality=85)
    out["unsupported_cmyk"] = np.frombuffer(bio.getvalue(), np.uint8)
    b = bytearray(encode(pic, "444", quality=85))               # a hand-built 4:4:0 header: luma sampled 1 x 2
    at = b.index(b"\xff\xc0")
    assert b[at + 9] == 3 and b[at + 11] == 0x11
    b[at + 11] = 0x12
    out["unsupported_440"] = np.frombuffer(bytes(b), np.uint8)
    for key in ("progressive", "cmyk", "440"):
        im = jpeg.JpegImage(out["unsupported_" + key].tobytes())
        assert not im.supported, key
        print("unsupported %-12s %s" % (key, im.reason))

    path = os.path.join(HERE, "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d bytes -> %s" % (len(cases), os.path.getsize(path), path))


if __name__ == "__main__":
    main()
