"""Shared by tests/test_jpeg_prog_cpu.py and tests/test_gpu_jpeg_prog.py: the progressive fixture files of
tests/golden/jpeg_prog_cases.npz (written by tests/golden/make_golden_jpeg_prog.py; ``rgb`` is what the reference's
``Image.open(f).convert('RGB')`` gave), the input records of tests/jpeg_prog_host.cpp, and its damaged scans."""
import os
import struct

import numpy as np

from helpers import ROOT
from instaorder_amd import jpeg

GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_prog_cases.npz")
# constants of tests/jpeg_prog_host.cpp
EVERY_BYTE, STRIDE, MUTATIONS = 4096, 16, 64

_cache = {}


def load():
    """(names, {name: (file bytes, rgb uint8 [H, W, 3])}, {kind: bytes of a file the device refuses}); loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        names = [str(n) for n in z["names"]]
        _cache["names"] = names
        _cache["cases"] = {n: (z["file_%d" % k].tobytes(), z["rgb_%d" % k]) for k, n in enumerate(names)}
        _cache["unsupported"] = {k[len("unsupported_"):]: z[k].tobytes() for k in z.files if k.startswith("unsupported_")}
    return _cache["names"], _cache["cases"], _cache["unsupported"]


def image(name):
    return jpeg.JpegImage(load()[1][name][0], name=name, progressive=True)


def mutated(data, m):
    """mutation m of tests/jpeg_prog_host.cpp (that of tests/jpeg_entropy_host.cpp)"""
    r = ((m + 1) * 2654435761) & 0xFFFFFFFF
    d = bytearray(data)
    d[r % len(d)] = (r >> 8) & 255
    return bytes(d)


def checksum(coef):
    """the coefficient checksum of the host programs: sum = sum * 31 + value over the uint16 values, mod 2^32"""
    c = np.ascontiguousarray(coef, np.int16).reshape(-1).view(np.uint16).astype(np.uint64)
    w = np.concatenate([np.cumprod(np.full(c.size - 1, 31, np.uint32), dtype=np.uint32)[::-1], [1]]).astype(np.uint64)
    return int((c * w).sum() & np.uint64(0xFFFFFFFF))


def image_file(im):
    """the input record of tests/jpeg_prog_host.cpp for one progressive image"""
    hs, vs = im.luma_sampling
    pool, scans = {}, b""
    for n, sc in enumerate(im.scans):
        tabs = [-1, -1, -1]
        for j, t in enumerate(sc.tables):
            if t is not None:
                tabs[j] = pool.setdefault(t, len(pool))
        scans += struct.pack("<11i", len(im.scan_bytes(n)), len(sc.comps), sc.comps[0], sc.ss, sc.se, sc.ah, sc.al,
                             sc.restart_interval, *tabs)
    head = struct.pack("<8i", 0x4a505047, im.W, im.H, len(im.components), hs, vs, len(pool), len(im.scans))
    tables = b"".join(cnt + sy + b"\0" * (256 - len(sy)) for cnt, sy in sorted(pool, key=pool.get))
    return head + tables + scans + b"".join(im.scan_bytes(n) for n in range(len(im.scans)))


def total_scan_bytes(im):
    return sum(len(im.scan_bytes(n)) for n in range(len(im.scans)))
