"""Shared by tests/test_png_cpu.py and tests/test_gpu_png.py: PNG files written here with ``zlib`` and ``struct`` so that
every property is forced (the filter type of each row, the compression strategy, the IDAT split), hand-made DEFLATE streams
(a fixed-Huffman writer) for what zlib never emits, the damaged streams -- a fixed list of truncations, seeded single-byte
mutations and one stream per status word -- that tests/png_inflate_host.cpp runs under the sanitizers, and the fixture
files of tests/golden/png_cases.npz (written by Pillow's encoder, tests/golden/make_golden_png.py)."""
import os
import struct
import zlib

import numpy as np

from helpers import ROOT
from instaorder_amd import png

GOLDEN = os.path.join(ROOT, "tests", "golden", "png_cases.npz")
FORMS = {"rgb": (2, 8, 3), "rgba": (6, 8, 4), "gray": (0, 8, 1), "gray16": (0, 16, 1)}    # colour type, depth, channels

_cache = {}


def load():
    """(names, {name: (file bytes, Pillow's decoded array)}, {kind: bytes of an unsupported file}); loaded once"""
    if not _cache:
        z = np.load(GOLDEN)
        names = [str(n) for n in z["names"]]
        _cache["names"] = names
        _cache["cases"] = {n: (z["file_%d" % k].tobytes(), z["ref_%d" % k]) for k, n in enumerate(names)}
        _cache["unsupported"] = {k[len("unsupported_"):]: z[k].tobytes() for k in z.files if k.startswith("unsupported_")}
    return _cache["names"], _cache["cases"], _cache["unsupported"]


# ---- pictures and files ---------------------------------------------------------------------------------------------------
def picture(H, W, form="rgb", seed=0):
    """a smooth picture with low-amplitude noise (noise alone does not compress: zlib stores it whatever the strategy):
    uint8 [H, W, C], or uint16 [H, W, 1] for gray16"""
    C = FORMS[form][2]
    rng = np.random.RandomState(seed)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    v = 3 * x + 2 * y + 40 * c + rng.randint(0, 4, (H, W, C))
    if form == "gray16":
        return ((v * 37) % 65536).astype(np.uint16)
    return (v % 256).astype(np.uint8)


def sample_bytes(px):
    """[H, W, C] samples -> uint8 [H, rowbytes] as the file stores them (16-bit samples big-endian)"""
    H = px.shape[0]
    if px.dtype == np.uint16:
        return px.astype(">u2").view(np.uint8).reshape(H, -1)
    return np.ascontiguousarray(px).reshape(H, -1)


def filtered(rows, bpp, filters):
    """uint8 [H, rowbytes] -> the scanlines with their filter bytes, uint8 [H, 1 + rowbytes]; filters: one type per row"""
    H, rb = rows.shape
    cur = rows.astype(np.int32)
    up = np.concatenate([np.zeros((1, rb), np.int32), cur[:-1]])
    left = np.concatenate([np.zeros((H, bpp), np.int32), cur[:, :-bpp]], 1) if rb > bpp else np.zeros((H, rb), np.int32)
    upleft = np.concatenate([np.zeros((H, bpp), np.int32), up[:, :-bpp]], 1) if rb > bpp else np.zeros((H, rb), np.int32)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    preds = [np.zeros_like(cur), left, up, (left + up) >> 1, paeth]
    out = np.zeros((H, 1 + rb), np.uint8)
    for y in range(H):
        out[y, 0] = filters[y]
        out[y, 1:] = (cur[y] - preds[filters[y] if filters[y] <= 4 else 0][y]) & 255
    return out


def chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(ctype + body) & 0xFFFFFFFF)


def png_file(H, W, form, zstream, idat=None, extra=()):
    """a PNG file around a zlib stream.  idat: None (one chunk), an int (chunks of that many bytes) or "mid" (two halves);
    extra: ancillary chunks (type, body) in front of the data"""
    ct, depth, _ = FORMS[form]
    if idat is None:
        parts = [zstream]
    elif idat == "mid":
        parts = [zstream[:len(zstream) // 2], zstream[len(zstream) // 2:]]
    else:
        parts = [zstream[i:i + idat] for i in range(0, len(zstream), idat)]
    return (png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ct, 0, 0, 0))
            + b"".join(chunk(t, b) for t, b in extra) + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_every=0):
    """a zlib stream of ``raw``; flush_every: Z_FULL_FLUSH after every so many bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
    if not flush_every:
        return c.compress(raw) + c.flush()
    out = b""
    for i in range(0, len(raw), flush_every):
        out += c.compress(raw[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def row_filters(H, filters, seed=0):
    if filters == "mix":
        return list(np.random.RandomState(1000 + seed).randint(0, 5, H))
    return [int(filters)] * H


def build(H, W, form="rgb", filters="mix", seed=0, px=None, idat=None, extra=(), name=None, **zopts):
    """(PngImage, expected array): a file of ``picture(H, W, form, seed)`` (or of ``px``) with the given filter type on
    every row ("mix": a seeded type per row) and ``deflate(**zopts)``"""
    px = picture(H, W, form, seed) if px is None else px
    depth, C = FORMS[form][1], FORMS[form][2]
    rows = sample_bytes(px)
    lines = filtered(rows, C * depth // 8, row_filters(H, filters, seed))
    if "flush_rows" in zopts:
        zopts = dict(zopts)
        zopts["flush_every"] = zopts.pop("flush_rows") * lines.shape[1]
    data = png_file(H, W, form, deflate(lines.tobytes(), **zopts), idat=idat, extra=extra)
    im = png.PngImage(data, name=name or "%dx%d_%s_%s" % (H, W, form, filters))
    return im, expected(px, form)


def expected(px, form):
    if form == "gray16":
        return px[:, :, 0].astype(np.uint16)
    if form == "gray":
        return np.repeat(px, 3, axis=2)
    return np.ascontiguousarray(px[:, :, :3])


# ---- a fixed-Huffman DEFLATE writer -------------------------------------------------------------------------------------------
class Bits(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                                     # n bits, lowest first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                                    # a Huffman code: highest bit first
        self.put(int("{:0{}b}".format(c, n)[::-1], 2), n)

    def lit(self, sym):                                      # the fixed literal/length code
        if sym < 144:
            self.code(0x30 + sym, 8)
        elif sym < 256:
            self.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.code(sym - 256, 7)
        else:
            self.code(0xC0 + sym - 280, 8)

    def match(self, length, dist):
        ls = max(i for i in range(29) if png._LEN_BASE[i] <= length and (i != 28 or length == 258))
        self.lit(257 + ls)
        self.put(length - png._LEN_BASE[ls], png._LEN_EXTRA[ls])
        ds = max(i for i in range(30) if png._DIST_BASE[i] <= dist)
        self.code(ds, 5)
        self.put(dist - png._DIST_BASE[ds], png._DIST_EXTRA[ds])

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def stored(self, data, final=0):
        self.put(final, 1)
        self.put(0, 2)
        self.align()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data

    def bytes(self):
        self.align()
        return bytes(self.out)


def zwrap(deflate_bytes, raw):
    return b"\x78\x01" + deflate_bytes + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


def distance_32768():
    """(PngImage, expected): gray, 1024 row bytes, 64 rows that repeat with a period of 32 rows -- every match of the
    second half has distance exactly 32768, which zlib's own encoder never emits (its window stops 262 bytes short)"""
    W, H = 1023, 64
    half = np.random.RandomState(5).randint(0, 256, (32, W, 1)).astype(np.uint8)
    px = np.concatenate([half, half])
    lines = filtered(sample_bytes(px), 1, [0] * H).tobytes()
    b = Bits()
    b.stored(lines[:32768])
    b.put(1, 1)
    b.put(1, 2)
    for ln in [258] * 126 + [257, 3]:
        b.match(ln, 32768)
    b.lit(256)
    im = png.PngImage(png_file(H, W, "gray", zwrap(b.bytes(), lines)), name="distance_32768")
    return im, expected(px, "gray")


def fibonacci_bytes():
    """bytes whose 20 values occur with the frequencies 2, 3, 5, 8, ..., rarest first.  In a gray image of one very long
    row the first block of a Z_HUFFMAN_ONLY stream then counts end-of-block once, the filter byte once and these values:
    a Fibonacci series without ties, whose Huffman tree is a chain that zlib cuts at its 15-bit limit"""
    fib = [2, 3]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    return np.concatenate([np.full(f, 40 + 7 * k, np.uint8) for k, f in enumerate(fib)])


# ---- damaged streams ------------------------------------------------------------------------------------------------------
BASE = dict(H=4, W=7, form="gray")           # the image of the hand-made streams: 32 inflated bytes
N_MUTATIONS = 120


def _base_lines():
    px = picture(BASE["H"], BASE["W"], "gray", seed=9)
    return px, filtered(sample_bytes(px), 1, [1, 2, 3, 4]).tobytes()


def per_status():
    """{status: PngImage} with one hand-made stream per status word, over the BASE image"""
    px, lines = _base_lines()
    good = png.PngImage(png_file(BASE["H"], BASE["W"], "gray", zlib.compress(lines)), name="base")
    pad = b"\0" * 8
    out = {0: good}
    out[1] = good.with_stream(b"\x07" + pad, name="status1")
    out[2] = good.with_stream(b"\x01" + struct.pack("<HH", 32, 32) + lines, name="status2")
    b = Bits()
    b.put(1, 1); b.put(2, 2); b.put(30, 5); b.put(0, 5); b.put(0, 4)          # HLIT = 30: 287 literal/length codes
    out[3] = good.with_stream(b.bytes() + pad, name="status3")
    b = Bits()
    b.put(1, 1); b.put(1, 2); b.lit(65); b.lit(257); b.code(30, 5)            # distance symbol 30
    out[4] = good.with_stream(b.bytes() + pad, name="status4")
    b = Bits()
    b.put(1, 1); b.put(1, 2); b.lit(65); b.match(3, 2); b.lit(256)            # distance 2 behind one byte
    out[5] = good.with_stream(b.bytes() + pad, name="status5")
    d = good.deflate_bytes()
    out[6] = good.with_stream(d[:len(d) // 2], name="status6")
    out[7] = good.with_stream(zlib.compress(lines[:-1])[2:-4], name="status7")
    out[8] = good.with_stream(d, adler=good.adler ^ 1, name="status8")
    bad = bytearray(lines)
    bad[8] = 5
    out[9] = good.with_stream(zlib.compress(bytes(bad))[2:-4], adler=zlib.adler32(bytes(bad)), name="status9")
    return out


def more_statuses():
    """further hand-made streams: [(PngImage, status)]"""
    px, lines = _base_lines()
    good = per_status()[0]
    out = [(good.with_stream(zlib.compress(lines + b"x")[2:-4], name="one byte more"), 7),
           (good.with_stream(b"", name="empty"), 6)]
    b = Bits()
    b.put(1, 1); b.put(1, 2); b.lit(286)
    out.append((good.with_stream(b.bytes() + b"\0" * 8, name="literal/length 286"), 4))
    b = Bits()                                               # a code-length code with one 1-bit code: incomplete
    b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(0, 4); b.put(1, 3)
    out.append((good.with_stream(b.bytes() + b"\0" * 8, name="incomplete code-length code"), 3))
    b = Bits()                                               # repeat-previous as the first code length
    b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(0, 4); b.put(1, 3); b.put(0, 3); b.put(0, 3); b.put(1, 3)
    b.put(1, 1)                                              # symbols 0 and 16 have the codes 0 and 1
    out.append((good.with_stream(b.bytes() + b"\0" * 8, name="repeat with nothing to repeat"), 3))
    return out


def mutated(data, m):
    """seeded single-byte mutation m"""
    r = ((m + 1) * 2654435761) & 0xFFFFFFFF
    d = bytearray(data)
    d[r % len(d)] = (r >> 8) & 255
    return bytes(d)


def truncations(n):
    return sorted({k for k in (0, 1, 2, 3, 5, n // 7, n // 3, n // 2, 2 * n // 3, n - 9, n - 5, n - 2, n - 1) if 0 <= k < n})


def fuzz_bases():
    """the three streams the host program and the GPU test damage: dynamic, fixed, and the memLevel=1 mix with stored blocks"""
    return [build(24, 31, "rgb", "mix", seed=1, name="fuzz_dynamic")[0],
            build(17, 23, "rgba", "mix", seed=2, strategy=zlib.Z_FIXED, name="fuzz_fixed")[0],
            build(40, 64, "rgb", 0, seed=3, mem_level=1, name="fuzz_mix")[0]]


def damaged():
    """[(label, PngImage)]: the fuzz bases intact, truncated and mutated, and the hand-made streams"""
    out = []
    for im in fuzz_bases():
        d = im.deflate_bytes()
        out.append((im.name, im))
        out += [("%s cut %d" % (im.name, k), im.with_stream(d[:k], name="%s cut %d" % (im.name, k))) for k in truncations(len(d))]
        out += [("%s mut %d" % (im.name, m), im.with_stream(mutated(d, m), name="%s mut %d" % (im.name, m)))
                for m in range(N_MUTATIONS)]
    out += [("status %d" % s, im) for s, im in sorted(per_status().items())]
    out += [(im.name, im) for im, s in more_statuses()]
    return out


def host_records(images):
    """the input file of tests/png_inflate_host.cpp: per stream <magic, bytes, expected output bytes> and the DEFLATE bytes"""
    return b"".join(struct.pack("<3i", 0x474e5089, len(im.deflate_bytes()), im.inflated_bytes) + im.deflate_bytes()
                    for im in images)


# ---- the images of the mixed GPU batch ----------------------------------------------------------------------------------------
def stream_cases():
    """[(PngImage, expected, check)] one image per stream property; check(stats) asserts that the property is there"""
    out = []

    def add(pair, check):
        out.append((pair[0], pair[1], check))

    add(build(150, 150, "rgb", 1, level=0, name="stored_only"),
        lambda s: s["stored"] >= 2 and s["fixed"] == s["dynamic"] == 0 and s["output_bytes"] > 65535)
    add(build(40, 40, "rgb", "mix", strategy=zlib.Z_FIXED, name="fixed_only"),
        lambda s: s["fixed"] >= 1 and s["stored"] == s["dynamic"] == 0)
    add(build(160, 160, "rgb", 4, seed=7, name="several_dynamic"), lambda s: s["dynamic"] >= 2 and s["stored"] == s["fixed"] == 0)
    add(build(96, 128, "rgb", 0, mem_level=1, name="memlevel1_mix"), lambda s: s["fixed"] >= 1 and s["stored"] >= 1)
    add(build(20, 30, "rgb", "mix", flush_rows=1, name="full_flush_rows"), lambda s: s["stored"] >= 20)
    add(build(30, 99, "gray", 0, px=np.full((30, 99, 1), 77, np.uint8), name="distance_1"),
        lambda s: s["min_distance"] == 1 and s["max_length"] == 258 and s["overlapping"] >= 2)
    half = picture(60, 150, "rgb", seed=4)
    add(build(120, 150, "rgb", 0, px=np.concatenate([half, half]), level=9, name="top_distance_code"),
        lambda s: s["max_distance"] > 24576)
    add(distance_32768(), lambda s: s["max_distance"] == 32768 and s["stored"] == 1 and s["fixed"] == 1)
    add(build(150, 150, "rgb", "mix", seed=6, name="ring_wraps"),
        lambda s: s["output_bytes"] > 65536 and s["max_distance"] > 0 and s["dynamic"] >= 1)
    fib = fibonacci_bytes()
    add(build(2, 17000, "gray", 0, px=fib[:34000].reshape(2, 17000, 1), strategy=zlib.Z_HUFFMAN_ONLY, name="code_15_bits"),
        lambda s: s["max_code_length"] == 15 and s["max_distance"] == 0)
    return out


def batch_cases():
    """[(PngImage, expected)] of the mixed batch of tests/test_gpu_png.py, without the stream-property images"""
    out = [build(1, 1, "rgb", "mix"), build(1, 37, "rgba", 4), build(41, 1, "gray16", "mix"), build(7, 5, "rgb", "mix"),
           build(6, 5, "gray", 3), build(1, 1, "gray16", 2)]
    band = png.UNFILTER_BAND
    out += [build(h, 9, "rgb", "mix", seed=h) for h in (band - 1, band, band + 1, 2 * band + 1)]
    out += [build(band + 1, 3, "gray16", 4, seed=8)]
    for form in ("rgb", "rgba", "gray", "gray16"):
        out += [build(9, 11, form, ft, seed=10 + k) for k, ft in enumerate([0, 1, 2, 3, 4, "mix"])]
    out.append(build(12, 13, "rgb", "mix", seed=20, idat=1, name="idat_1_byte"))
    out.append(build(12, 13, "rgba", "mix", seed=21, idat="mid", name="idat_mid"))
    out.append(build(8, 9, "gray", "mix", seed=22, extra=[(b"gAMA", struct.pack(">I", 45455)), (b"tRNS", b"\0\x07")],
                     name="ancillary"))
    return out
