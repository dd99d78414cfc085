"""Shared by tests/test_jpeg_cpu.py and tests/test_gpu_jpeg.py: the fixture files of tests/golden/jpeg_cases.npz (written by
tests/golden/make_golden_jpeg.py; ``rgb`` is what the reference's ``Image.open(f).convert('RGB')`` gave), and the damaged
streams -- the truncations and seeded mutations that tests/jpeg_entropy_host.cpp runs under the sanitizers."""
import os
import struct

import numpy as np

from helpers import ROOT
from instaorder_amd import jpeg

GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
# the three streams the host program and the GPU test damage: restart markers, 4:2:0 with long codes, grayscale
FUZZ = ["21x35_444_rst2", "33x47_420_q100", "40x24_gray_opt"]

_cache = {}


def load():
    """(names, {name: (file bytes, rgb uint8 [H, W, 3])}, {kind: bytes of an unsupported file}); loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        names = [str(n) for n in z["names"]]
        _cache["names"] = names
        _cache["cases"] = {n: (z["file_%d" % k].tobytes(), z["rgb_%d" % k]) for k, n in enumerate(names)}
        _cache["unsupported"] = {k[len("unsupported_"):]: z[k].tobytes() for k in z.files if k.startswith("unsupported_")}
    return _cache["names"], _cache["cases"], _cache["unsupported"]


def image(name):
    return jpeg.JpegImage(load()[1][name][0], name=name)


def mutated(data, m):
    """mutation m of tests/jpeg_entropy_host.cpp"""
    r = ((m + 1) * 2654435761) & 0xFFFFFFFF
    d = bytearray(data)
    d[r % len(d)] = (r >> 8) & 255
    return bytes(d)


def status_of(im):
    """(status the decoder must report, coefficient checksum of the host program or None)"""
    try:
        c = im.coefficients().reshape(-1).view(np.uint16).astype(np.uint64)
    except jpeg.JpegStreamError as e:
        return e.status, None
    w = np.concatenate([np.cumprod(np.full(c.size - 1, 31, np.uint32), dtype=np.uint32)[::-1], [1]]).astype(np.uint64)
    return 0, int((c * w).sum() & np.uint64(0xFFFFFFFF))


def stream_file(im):
    """the input record of tests/jpeg_entropy_host.cpp for one image"""
    hs, vs = im.luma_sampling
    nc = len(im.components)
    mw, mh = -(-im.W // (8 * hs)), -(-im.H // (8 * vs))
    ent = im.entropy_bytes()
    tabs = list(im.scan_tables) + [(0, 0)] * (3 - nc)
    head = struct.pack("<12i", 0x4a504547, len(ent), mw * mh, hs * vs, 1 if nc == 3 else 0, im.restart_interval,
                       *([t[0] for t in tabs] + [2 + t[1] for t in tabs]))
    blob = np.frombuffer(im.tables_blob(), np.uint8)
    counts, syms = blob[512:576].reshape(4, 16), blob[576:].reshape(4, 256)
    return head + b"".join(counts[t].tobytes() + syms[t].tobytes() for t in range(4)) + ent
