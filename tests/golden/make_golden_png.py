"""Writes tests/golden/png_cases.npz: small PNG files written by Pillow's own encoder (which chooses the filter of every
row adaptively) and what the reference's loads make of them -- ``np.array(Image.open(f).convert('RGB'))`` for the 8-bit
forms (datasets/occ_order_dataset.py:79), ``np.array(Image.open(f))`` for 16-bit gray -- so that the tests need no
Pillow.  Needs Pillow and NumPy:

    python tests/golden/make_golden_png.py

One file per unsupported form is kept too.  The script asserts that ``PngImage.to_host()`` agrees on every file.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, PngImagePlugin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from instaorder_amd import png  # noqa: E402


def picture(H, W, C, rng):
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return ((127 + 90 * np.sin(x / 5. + y / 9. + c) + rng.randn(H, W, C) * 6).clip(0, 255)).astype(np.uint8)


def save(img, **kw):
    bio = io.BytesIO()
    img.save(bio, "PNG", **kw)
    return bio.getvalue()


def main():
    rng = np.random.RandomState(20261020)
    cases = []
    for H, W in [(1, 1), (7, 5), (33, 47)]:
        cases.append(("%dx%d_rgb" % (H, W), save(Image.fromarray(picture(H, W, 3, rng)))))
    cases.append(("21x35_rgb_l9", save(Image.fromarray(picture(21, 35, 3, rng)), compress_level=9)))
    cases.append(("21x35_rgb_l1", save(Image.fromarray(picture(21, 35, 3, rng)), compress_level=1)))
    cases.append(("21x35_rgba", save(Image.fromarray(picture(21, 35, 4, rng)))))
    cases.append(("9x17_rgba", save(Image.fromarray(picture(9, 17, 4, rng)), optimize=True)))
    cases.append(("40x24_gray", save(Image.fromarray(picture(40, 24, 1, rng)[:, :, 0]))))
    cases.append(("5x64_gray", save(Image.fromarray(picture(5, 64, 1, rng)[:, :, 0]))))
    depth = (picture(30, 41, 1, rng)[:, :, 0].astype(np.uint16) * 257) * (rng.rand(30, 41) < 0.3)
    cases.append(("30x41_gray16", save(Image.fromarray(depth.astype(np.uint16)))))
    cases.append(("3x2_gray16", save(Image.fromarray((rng.randint(0, 65536, (3, 2))).astype(np.uint16)))))
    # ancillary chunks: tRNS on RGB and gray (Pillow keeps the mode), gAMA
    cases.append(("21x35_rgb_trns", save(Image.fromarray(picture(21, 35, 3, rng)), transparency=(1, 2, 3))))
    cases.append(("21x35_gray_trns", save(Image.fromarray(picture(21, 35, 1, rng)[:, :, 0]), transparency=7)))
    info = PngImagePlugin.PngInfo()
    info.add(b"gAMA", (45455).to_bytes(4, "big"))
    cases.append(("21x35_rgb_gama", save(Image.fromarray(picture(21, 35, 3, rng)), pnginfo=info)))
    out = {"names": np.array([c[0] for c in cases])}
    for k, (name, data) in enumerate(cases):
        img = Image.open(io.BytesIO(data))
        ref = np.array(img) if name.endswith("gray16") else np.array(img.convert("RGB"))
        im = png.PngImage(data, name=name)
        assert im.supported, (name, im.reason)
        assert ref.dtype == im.dtype and ref.shape == im.shape, (name, ref.dtype, ref.shape)
        assert np.array_equal(im.to_host(), ref), name
        out["file_%d" % k] = np.frombuffer(data, np.uint8)
        out["ref_%d" % k] = ref
    assert any("tRNS" in [t for t, _ in png.PngImage(d).chunks] for n, d in cases)
    assert any("gAMA" in [t for t, _ in png.PngImage(d).chunks] for n, d in cases)
    pal = Image.fromarray(picture(21, 35, 3, rng)).convert("P")
    unsupported = {"palette": save(pal)}
    # Pillow writes no 16-bit colour, 4-bit gray or Adam7: those files are written by hand around a zlib stream
    import struct
    import zlib

    def chunk(t, b):
        return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b) & 0xFFFFFFFF)

    def by_hand(depth, ct, interlace, raw):
        return (png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 35, 21, depth, ct, 0, 0, interlace))
                + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))

    unsupported["rgb16"] = by_hand(16, 2, 0, bytes(21 * (1 + 35 * 6)))
    unsupported["4bit_gray"] = by_hand(4, 0, 0, bytes(21 * (1 + 18)))
    unsupported["interlaced"] = by_hand(8, 2, 1, bytes(21 * (1 + 35 * 3) + 16))
    for kind, data in unsupported.items():
        im = png.PngImage(data, name=kind)
        assert not im.supported, kind
        out["unsupported_" + kind] = np.frombuffer(data, np.uint8)
    np.savez_compressed(os.path.join(HERE, "png_cases.npz"), **out)
    print("wrote %d cases, %d unsupported, %d file bytes" % (len(cases), len(unsupported), sum(len(d) for _, d in cases)))


if __name__ == "__main__":
    main()
