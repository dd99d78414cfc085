"""PNG images and 16-bit depth maps for the device input pipeline.

KINS / KITTI frames are 8-bit RGB PNG files and the KITTI ground-truth depth maps 16-bit grayscale ones; the reference
loads them with ``Image.open(fn).convert('RGB')`` (datasets/occ_order_dataset.py:79) and ``cv2.imread(f, -1)``.  A
``PngImage`` keeps the file's bytes instead: the chunks are parsed here (pure Python, no GPU needed), only the DEFLATE
stream and a descriptor are uploaded, and ``io_png_decode`` (csrc/png.hip) decodes in front of the render kernel
(``datasets.PairRenderer``) or of the depth metrics (``dense_eval``), next to the JPEG images and the encoded masks.

The rule (DESIGN.md "PNG images") is RFC 1950 / 1951 / 2083 with zlib's acceptance rules, all in integers:

1. Inflate: the concatenated IDAT payloads are one zlib stream; its DEFLATE bytes must yield exactly ``H * (1 + rowbytes)``
   bytes whose Adler-32 is the big-endian word at the end of the stream.
2. Unfilter: every scanline starts with a filter byte 0..4 (None, Sub, Up, Average, Paeth), applied per byte with the
   pixel to the left (``bpp`` bytes back), the byte above and the one above left, zero outside the image, modulo 256.
3. Pack: 8-bit RGB is copied, RGBA loses its alpha, gray is replicated to R = G = B -- uint8 [H, W, 3], exactly
   ``np.array(Image.open(f).convert('RGB'))``; 16-bit gray ("raw16") becomes uint16 [H, W] in host byte order, the
   values ``cv2.imread(f, -1)`` gives, and is not a picture: the renderer refuses it.

``PngImage.to_host()`` is that rule in NumPy and the contract of the kernels; ``PngImage.inflate_status()`` states the
inflate stage of csrc/png_inflate.h in Python, status word by status word.

The inflate stage runs in two ways with the same bytes and status words: one wave per image (``io_png_decode``) and one
stream on many waves from found block starts (``io_png_decode_par``, csrc/png_inflate_par.h), chosen by ``set_inflate``;
``PngImage.parallel_plan`` is the rule of the latter in Python.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import _lib, arena

SIGNATURE = b"\x89PNG\r\n\x1a\n"
STATUS = {1: "block type 3", 2: "a stored block whose length and complement disagree", 3: "an invalid code-length set",
          4: "an invalid literal/length or distance symbol", 5: "a distance reaching before the first output byte",
          6: "data exhausted before the end of the final block", 7: "the stream does not yield H * (1 + rowbytes) bytes",
          8: "Adler-32 mismatch", 9: "a filter byte above 4"}
UNFILTER_BAND = 64           # PNG_BAND_ROWS of csrc/png.hip: rows the skewed wavefront of the unfilter stage takes at once

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
              6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
_REV = np.array([int("{:015b}".format(i)[::-1], 2) for i in range(1 << 15)], np.int64)


class PngStreamError(ValueError):
    """the zlib stream of a well-formed file does not decode; ``status`` is the kernel's status word"""

    def __init__(self, status, name):
        ValueError.__init__(self, "PNG image %s: %s (status %d)" % (name, STATUS.get(status, "?"), status))
        self.status = status


def _code_table(lengths, kind):
    """15-bit lookup (index: the next 15 stream bits, first bit lowest) -> (length << 9) | symbol, 0 where no code starts,
    by zlib's inflate_table rules; None for a set it refuses.  kind: "codes" (the code-length code: must be complete),
    "lens" / "dists" (incomplete only as a single 1-bit code; "dists" may be empty)."""
    lengths = np.asarray(lengths, np.int64)
    count = np.bincount(lengths, minlength=16)
    tab = np.zeros(1 << 15, np.int32)
    if count[0] == lengths.size:
        return None if kind == "codes" else tab              # no distance codes at all is no error by itself
    left = 1
    for l in range(1, 16):
        left = (left << 1) - int(count[l])
        if left < 0:
            return None
    longest = int(np.nonzero(count[1:])[0].max()) + 1
    if left > 0 and (kind == "codes" or longest != 1):
        return None
    code = 0
    nxt = [0] * 16
    for l in range(1, 16):
        code = (code + int(count[l - 1] if l > 1 else 0)) << 1
        nxt[l] = code
    for sym, l in enumerate(lengths):
        l = int(l)
        if l:
            rev = int(_REV[nxt[l]]) >> (15 - l)
            nxt[l] += 1
            tab[rev::1 << l] = (l << 9) | sym
    return tab


_FIXED = []


def _fixed_tables():
    if not _FIXED:
        _FIXED.append(_code_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "lens"))
        _FIXED.append(_code_table([5] * 32, "dists"))
    return _FIXED


def inflate_walk(data, expected=None, keep=True, boundaries=None):
    """The inflate loop of csrc/png_inflate.h in Python over raw DEFLATE bytes: (status, bytes produced or None, stats).
    ``expected``: the byte count the stream must yield (status 7 otherwise; None: any).  stats: dict(stored, fixed,
    dynamic, min_distance, max_distance, max_length, overlapping, max_code_length, output_bytes).  ``boundaries``: a list
    that receives (bit, bytes produced so far) behind every block.  Slow: small files."""
    data = bytes(data)
    nb = len(data)
    st = dict(stored=0, fixed=0, dynamic=0, min_distance=0, max_distance=0, max_length=0, overlapping=0,
              max_code_length=0, output_bytes=0)
    out = bytearray()
    n_out = 0
    buf, cnt, pos = 0, 0, 0

    def done(status):
        st["output_bytes"] = n_out
        return status, (bytes(out) if keep and status == 0 else None), st

    def over():
        return 8 * pos - cnt > 8 * nb

    while True:
        while cnt < 3:
            buf |= (data[pos] if pos < nb else 0) << cnt
            pos += 1
            cnt += 8
        final, kind = buf & 1, (buf >> 1) & 3
        buf >>= 3
        cnt -= 3
        if over():
            return done(6)
        if kind == 3:
            return done(1)
        if kind == 0:
            buf >>= cnt & 7
            cnt -= cnt & 7
            while cnt < 32:
                buf |= (data[pos] if pos < nb else 0) << cnt
                pos += 1
                cnt += 8
            ln, nln = buf & 0xFFFF, (buf >> 16) & 0xFFFF
            buf >>= 32
            cnt -= 32
            if over():
                return done(6)
            if ln != nln ^ 0xFFFF:
                return done(2)
            pos -= cnt >> 3
            buf, cnt = 0, 0
            if pos + ln > nb:
                return done(6)
            if expected is not None and n_out + ln > expected:
                return done(7)
            st["stored"] += 1
            if keep:
                out += data[pos:pos + ln]
            n_out += ln
            pos += ln
        else:
            if kind == 1:
                st["fixed"] += 1
                lit, dist = _fixed_tables()
            else:
                while cnt < 14:
                    buf |= (data[pos] if pos < nb else 0) << cnt
                    pos += 1
                    cnt += 8
                nlen, ndist, ncode = (buf & 31) + 257, ((buf >> 5) & 31) + 1, ((buf >> 10) & 15) + 4
                buf >>= 14
                cnt -= 14
                if over():
                    return done(6)
                if nlen > 286 or ndist > 30:
                    return done(3)
                cl = [0] * 19
                for i in range(ncode):
                    while cnt < 3:
                        buf |= (data[pos] if pos < nb else 0) << cnt
                        pos += 1
                        cnt += 8
                    cl[_CL_ORDER[i]] = buf & 7
                    buf >>= 3
                    cnt -= 3
                if over():
                    return done(6)
                ctab = _code_table(cl, "codes")
                if ctab is None:
                    return done(3)
                lens = []
                while len(lens) < nlen + ndist:
                    while cnt < 22:
                        buf |= (data[pos] if pos < nb else 0) << cnt
                        pos += 1
                        cnt += 8
                    e = int(ctab[buf & 0x7FFF])
                    l, sym = e >> 9, e & 511                             # the code is complete: every pattern decodes
                    buf >>= l
                    cnt -= l
                    if sym < 16:
                        if over():
                            return done(6)
                        lens.append(sym)
                        continue
                    if sym == 16:
                        rep, val = 3 + (buf & 3), (lens[-1] if lens else -1)
                        l = 2
                    elif sym == 17:
                        rep, val, l = 3 + (buf & 7), 0, 3
                    else:
                        rep, val, l = 11 + (buf & 127), 0, 7
                    buf >>= l
                    cnt -= l
                    if over():
                        return done(6)
                    if val < 0 or len(lens) + rep > nlen + ndist:
                        return done(3)
                    lens += [val] * rep
                if lens[256] == 0:
                    return done(3)
                lit = _code_table(lens[:nlen], "lens")
                dist = _code_table(lens[nlen:], "dists") if lit is not None else None
                if lit is None or dist is None:
                    return done(3)
                st["dynamic"] += 1
            while True:
                while cnt < 48:
                    buf |= (data[pos] if pos < nb else 0) << cnt
                    pos += 1
                    cnt += 8
                e = int(lit[buf & 0x7FFF])
                if e == 0:
                    return done(6 if 8 * nb - (8 * pos - cnt) < 15 else 4)     # a longer code might have followed
                l, sym = e >> 9, e & 511
                buf >>= l
                cnt -= l
                if over():
                    return done(6)
                if l > st["max_code_length"]:
                    st["max_code_length"] = l
                if sym < 256:
                    if expected is not None and n_out >= expected:
                        return done(7)
                    if keep:
                        out.append(sym)
                    n_out += 1
                    continue
                if sym == 256:
                    break
                if sym > 285:
                    return done(4)
                ln = _LEN_BASE[sym - 257] + (buf & ((1 << _LEN_EXTRA[sym - 257]) - 1))
                buf >>= _LEN_EXTRA[sym - 257]
                cnt -= _LEN_EXTRA[sym - 257]
                e = int(dist[buf & 0x7FFF])
                if e == 0:
                    return done(6 if 8 * nb - (8 * pos - cnt) < 15 else 4)     # a longer code might have followed
                l, ds = e >> 9, e & 511
                buf >>= l
                cnt -= l
                if over():
                    return done(6)
                if l > st["max_code_length"]:
                    st["max_code_length"] = l
                if ds > 29:
                    return done(4)
                d = _DIST_BASE[ds] + (buf & ((1 << _DIST_EXTRA[ds]) - 1))
                buf >>= _DIST_EXTRA[ds]
                cnt -= _DIST_EXTRA[ds]
                if over():
                    return done(6)
                if d > n_out:
                    return done(5)
                if expected is not None and n_out + ln > expected:
                    return done(7)
                st["min_distance"] = d if st["min_distance"] == 0 else min(st["min_distance"], d)
                st["max_distance"] = max(st["max_distance"], d)
                st["max_length"] = max(st["max_length"], ln)
                st["overlapping"] += d < ln
                if keep:
                    if d >= ln:
                        out += out[n_out - d:n_out - d + ln]
                    else:
                        seg = bytes(out[n_out - d:])
                        out += (seg * (ln // d + 1))[:ln]
                n_out += ln
        if boundaries is not None:
            boundaries.append((8 * pos - cnt, n_out))
        if final:
            break
    if expected is not None and n_out != expected:
        return done(7)
    return done(0)


# ---- parallel inflate: the rule of csrc/png_inflate_par.h ---------------------------------------------------------------
PAR_MIN_CHUNK, PAR_MAX_CHUNK, PAR_MAX_CHUNKS = 256, 1 << 20, 65535
INFO_NOT_CLEAN, INFO_CHAIN_OF_ONE = 1 << 16, 1 << 17
EXIT_NONE, EXIT_FINAL, EXIT_LINK, EXIT_STATUS = 0, 1, 2, 3


def _dynamic_header(data, bit):
    """A dynamic-block header at ``bit`` (its BFINAL bit) by the rules of ``inflate_walk``: (literal/length table, distance
    table, the bit behind the header), or the status word."""
    nb = len(data)
    pos = bit >> 3
    buf, cnt = 0, 0

    def need(n):
        nonlocal buf, cnt, pos
        while cnt < n:
            buf |= (data[pos] if pos < nb else 0) << cnt
            pos += 1
            cnt += 8

    def take(n):
        nonlocal buf, cnt
        v = buf & ((1 << n) - 1)
        buf >>= n
        cnt -= n
        return v

    def over():
        return 8 * pos - cnt > 8 * nb

    need(8)
    take(bit & 7)
    need(17)
    take(1)
    if take(2) != 2:
        return 1
    nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
    if over():
        return 6
    if nlen > 286 or ndist > 30:
        return 3
    cl = [0] * 19
    for i in range(ncode):
        need(3)
        cl[_CL_ORDER[i]] = take(3)
    if over():
        return 6
    ctab = _code_table(cl, "codes")
    if ctab is None:
        return 3
    lens = []
    while len(lens) < nlen + ndist:
        need(22)
        e = int(ctab[buf & 0x7FFF])
        take(e >> 9)
        sym = e & 511
        if sym < 16:
            rep, val = 1, sym
        elif sym == 16:
            rep, val = 3 + take(2), (lens[-1] if lens else -1)
        elif sym == 17:
            rep, val = 3 + take(3), 0
        else:
            rep, val = 11 + take(7), 0
        if over():
            return 6
        if val < 0 or len(lens) + rep > nlen + ndist:
            return 3
        lens += [val] * rep
    if lens[256] == 0:
        return 3
    lit = _code_table(lens[:nlen], "lens")
    dist = _code_table(lens[nlen:], "dists") if lit is not None else None
    if lit is None or dist is None:
        return 3
    return lit, dist, 8 * pos - cnt


def dynamic_header_bits(data):
    """every bit of ``data`` at which a complete dynamic-block header parses (search of csrc/png_inflate_par.h), ascending.
    A vectorised necessary condition first -- BTYPE 2, HLIT <= 286, HDIST <= 30, a code-length code with Kraft sum 1 --
    then the parse itself."""
    data = bytes(data)
    nb = len(data)
    if nb == 0:
        return []
    bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")
    bits = np.concatenate([bits, np.zeros(96, np.uint8)]).astype(np.int64)
    p = np.nonzero((bits[1:8 * nb + 1] == 0) & (bits[2:8 * nb + 2] == 1))[0]

    def field(at, n):
        v = np.zeros(p.size, np.int64)
        for i in range(n):
            v |= bits[p + at + i] << i
        return v

    keep = (field(3, 5) <= 29) & (field(8, 5) <= 29)
    p = p[keep]
    ncode = field(13, 4) + 4
    kraft = np.zeros(p.size, np.int64)
    for i in range(19):
        v = field(17 + 3 * i, 3)
        kraft += np.where((i < ncode) & (v > 0), 128 >> v, 0)
    return [int(q) for q in p[kraft == 128] if not isinstance(_dynamic_header(data, int(q)), int)]


def _chunk_walk(data, start, expected, cands, chunk_bits):
    """One chunk's decode from bit ``start`` (count and store pass of csrc/png_inflate_par.h at once): dict(exit, exit_bit,
    n, reach, status, next, syms: the 16-bit symbols as a list, blocks: [stored, fixed, dynamic], copied: markers that a
    match copied from inside the chunk).  cands: {candidate bit: chunk}."""
    nb = len(data)
    pos = start >> 3
    buf, cnt = 0, 0
    while cnt < 8:
        buf |= (data[pos] if pos < nb else 0) << cnt
        pos += 1
        cnt += 8
    buf >>= start & 7
    cnt -= start & 7
    syms = []
    blocks = [0, 0, 0]
    rec = dict(exit=EXIT_NONE, exit_bit=0, n=0, reach=0, status=0, next=-1, syms=syms, blocks=blocks, copied=0)

    def end(kind, status=0):
        rec.update(exit=kind, status=status, exit_bit=8 * pos - cnt, n=len(syms))
        return rec

    while True:
        while cnt < 3:
            buf |= (data[pos] if pos < nb else 0) << cnt
            pos += 1
            cnt += 8
        final, kind = buf & 1, (buf >> 1) & 3
        buf >>= 3
        cnt -= 3
        if 8 * pos - cnt > 8 * nb:
            return end(EXIT_STATUS, 6)
        if kind == 3:
            return end(EXIT_STATUS, 1)
        if kind == 0:
            buf >>= cnt & 7
            cnt -= cnt & 7
            while cnt < 32:
                buf |= (data[pos] if pos < nb else 0) << cnt
                pos += 1
                cnt += 8
            ln, nln = buf & 0xFFFF, (buf >> 16) & 0xFFFF
            buf >>= 32
            cnt -= 32
            if 8 * pos - cnt > 8 * nb:
                return end(EXIT_STATUS, 6)
            if ln != nln ^ 0xFFFF:
                return end(EXIT_STATUS, 2)
            pos -= cnt >> 3
            buf, cnt = 0, 0
            if pos + ln > nb:
                return end(EXIT_STATUS, 6)
            if len(syms) + ln > expected:
                return end(EXIT_STATUS, 7)
            syms += data[pos:pos + ln]
            pos += ln
            blocks[0] += 1
        else:
            if kind == 1:
                lit, dist = _fixed_tables()
            else:
                h = _dynamic_header(data, 8 * pos - cnt - 3)
                if isinstance(h, int):
                    return end(EXIT_STATUS, h)               # (exit_bit is the contract of "final" and "link" exits only)
                lit, dist, at = h
                pos, buf, cnt = at >> 3, 0, 0
                while cnt < 8:
                    buf |= (data[pos] if pos < nb else 0) << cnt
                    pos += 1
                    cnt += 8
                buf >>= at & 7
                cnt -= at & 7
            blocks[kind] += 1
            while True:
                while cnt < 48:
                    buf |= (data[pos] if pos < nb else 0) << cnt
                    pos += 1
                    cnt += 8
                e = int(lit[buf & 0x7FFF])
                if e == 0:
                    return end(EXIT_STATUS, 6 if 8 * nb - (8 * pos - cnt) < 15 else 4)
                l, sym = e >> 9, e & 511
                buf >>= l
                cnt -= l
                if 8 * pos - cnt > 8 * nb:
                    return end(EXIT_STATUS, 6)
                if sym < 256:
                    if len(syms) >= expected:
                        return end(EXIT_STATUS, 7)
                    syms.append(sym)
                    continue
                if sym == 256:
                    break
                if sym > 285:
                    return end(EXIT_STATUS, 4)
                x = _LEN_EXTRA[sym - 257]
                ln = _LEN_BASE[sym - 257] + (buf & ((1 << x) - 1))
                buf >>= x
                cnt -= x
                e = int(dist[buf & 0x7FFF])
                if e == 0:
                    return end(EXIT_STATUS, 6 if 8 * nb - (8 * pos - cnt) < 15 else 4)
                l, ds = e >> 9, e & 511
                buf >>= l
                cnt -= l
                if 8 * pos - cnt > 8 * nb:
                    return end(EXIT_STATUS, 6)
                if ds > 29:
                    return end(EXIT_STATUS, 4)
                x = _DIST_EXTRA[ds]
                d = _DIST_BASE[ds] + (buf & ((1 << x) - 1))
                buf >>= x
                cnt -= x
                if 8 * pos - cnt > 8 * nb:
                    return end(EXIT_STATUS, 6)
                n_out = len(syms)
                if d > n_out:
                    rec["reach"] = max(rec["reach"], d - n_out)
                if n_out + ln > expected:
                    return end(EXIT_STATUS, 7)
                first = []                                   # the match's first min(d, ln) symbols
                for k in range(min(d, ln)):
                    src = n_out - d + k
                    if src < 0:
                        first.append(0x8000 | (-src - 1))
                    else:
                        first.append(syms[src])
                        rec["copied"] += syms[src] >= 0x8000
                syms += (first * (ln // len(first) + 1))[:ln]
        b = 8 * pos - cnt
        if final:
            return end(EXIT_FINAL)
        c = cands.get(b)
        if c is not None and c == b // chunk_bits:
            rec["next"] = c
            return end(EXIT_LINK)


def _unfilter(raw, H, rowbytes, bpp):
    """stage 2 on the inflated bytes (uint8 [H * (1 + rowbytes)]) -> uint8 [H, rowbytes]; None when a filter byte is above
    4.  One NumPy step per anti-diagonal of pixels: the skewed wavefront of the kernel."""
    rows = raw.reshape(H, 1 + rowbytes)
    ft = rows[:, 0].astype(np.int64)
    if ft.size and ft.max() > 4:
        return None
    W = rowbytes // bpp
    src = rows[:, 1:].reshape(H, W, bpp).astype(np.int32)
    if not np.any(ft > 2):                                   # None / Sub / Up only: whole rows at a time
        out = np.zeros((H + 1, W, bpp), np.int32)
        for y in range(H):
            if ft[y] == 1:
                out[y + 1] = np.cumsum(src[y], axis=0) & 255
            elif ft[y] == 2:
                out[y + 1] = (src[y] + out[y]) & 255
            else:
                out[y + 1] = src[y]
        return out[1:].astype(np.uint8).reshape(H, rowbytes)
    out = np.zeros((H + 1, W + 1, bpp), np.int32)            # a zero row above and a zero column to the left
    ftc = ft[:, None]
    for s in range(H + W - 1):
        ys = np.arange(max(0, s - W + 1), min(H, s + 1))
        xs = s - ys
        a, b, c = out[ys + 1, xs], out[ys, xs + 1], out[ys, xs]
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        t = ftc[ys]
        pred = np.where(t == 1, a, np.where(t == 2, b, np.where(t == 3, (a + b) >> 1, np.where(t == 4, paeth, 0))))
        out[ys + 1, xs + 1] = (src[ys, xs] + pred) & 255
    return out[1:, 1:].astype(np.uint8).reshape(H, rowbytes)


class PngImage(object):
    """One PNG file, parsed but not decoded.  Stands in for a uint8 [H, W, 3] array (a uint16 [H, W] one in the raw16
    form) where the consumers only look at ``shape`` / ``dtype``; ``supported`` says whether the device decoder takes it
    (``reason`` why not)."""

    def __init__(self, data, name=None):
        self.data = bytes(data)
        self.name = name if name is not None else "<%d bytes>" % len(self.data)
        self.reason = None
        self.H = self.W = 0
        self.bit_depth = self.colour_type = self.interlace = 0
        self.channels = 0                # samples per pixel in the file
        self.chunks = []                 # (type, payload length) in file order
        self.adler = 0
        self.nbytes_stream = 0           # the zlib stream: header, DEFLATE bytes, Adler-32
        self._deflate = b""
        self._parse()

    @classmethod
    def open(cls, path):
        with open(path, "rb") as f:
            return cls(f.read(), name=str(path))

    # ---- the array surface -------------------------------------------------------------------------------------------
    @property
    def raw16(self):
        return self.colour_type == 0 and self.bit_depth == 16

    @property
    def shape(self):
        return (self.H, self.W) if self.raw16 else (self.H, self.W, 3)

    @property
    def ndim(self):
        return 2 if self.raw16 else 3

    @property
    def dtype(self):
        return np.dtype(np.uint16 if self.raw16 else np.uint8)

    @property
    def supported(self):
        return self.reason is None

    @property
    def nbytes_compressed(self):
        return len(self.data)

    @property
    def bpp(self):
        """bytes per pixel in the file: the distance of the Sub / Average / Paeth filters"""
        return max(1, self.channels * self.bit_depth // 8)

    @property
    def rowbytes(self):
        return (self.W * self.channels * self.bit_depth + 7) // 8

    @property
    def inflated_bytes(self):
        return self.H * (1 + self.rowbytes)

    @property
    def out_bytes(self):
        return self.H * self.W * (2 if self.raw16 else 3)

    def _no(self, reason):
        if self.reason is None:
            self.reason = reason

    # ---- chunks ------------------------------------------------------------------------------------------------------
    def _parse(self):
        b = self.data
        n = len(b)
        if b[:8] != SIGNATURE:
            raise ValueError("PNG %s: no PNG signature" % self.name)
        p = 8
        idat = []
        seen_ihdr = False
        while p < n:
            if p + 12 > n:
                raise ValueError("PNG %s: the file ends inside a chunk header (byte %d)" % (self.name, p))
            L, ctype = struct.unpack_from(">I4s", b, p)
            if p + 12 + L > n:
                raise ValueError("PNG %s: chunk %r of length %d runs past the end of the file" % (self.name, ctype, L))
            body = b[p + 8:p + 8 + L]
            crc = struct.unpack_from(">I", b, p + 8 + L)[0]
            p += 12 + L
            if not seen_ihdr and ctype != b"IHDR":
                raise ValueError("PNG %s: the first chunk is %r, not IHDR" % (self.name, ctype))
            if ctype in (b"IHDR", b"IDAT") and zlib.crc32(ctype + body) & 0xFFFFFFFF != crc:
                raise ValueError("PNG %s: bad CRC of an %s chunk" % (self.name, ctype.decode()))
            self.chunks.append((ctype.decode("latin-1"), L))
            if ctype == b"IHDR":
                if seen_ihdr or L != 13:
                    raise ValueError("PNG %s: malformed IHDR" % self.name)
                seen_ihdr = True
                self.W, self.H, self.bit_depth, self.colour_type, comp, filt, self.interlace = struct.unpack(">IIBBBBB", body)
            elif ctype == b"IDAT":
                idat.append(body)
            elif ctype == b"IEND":
                break
        if not seen_ihdr or not idat:
            raise ValueError("PNG %s: no IHDR or no IDAT chunk" % self.name)
        if self.W == 0 or self.H == 0 or comp != 0 or filt != 0 or self.interlace > 1:
            raise ValueError("PNG %s: invalid IHDR (%d x %d, compression %d, filter %d, interlace %d)"
                             % (self.name, self.W, self.H, comp, filt, self.interlace))
        self.channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}.get(self.colour_type, 0)
        if self.channels == 0 or self.bit_depth not in (1, 2, 4, 8, 16):
            raise ValueError("PNG %s: colour type %d with bit depth %d" % (self.name, self.colour_type, self.bit_depth))
        stream = b"".join(idat)
        self.nbytes_stream = len(stream)
        if len(stream) < 6:
            raise ValueError("PNG %s: a zlib stream of %d bytes" % (self.name, len(stream)))
        cmf, flg = stream[0], stream[1]
        if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 0x20 or (cmf * 256 + flg) % 31:
            raise ValueError("PNG %s: invalid zlib header %02x %02x" % (self.name, cmf, flg))
        self._deflate = stream[2:-4]
        self.adler = struct.unpack(">I", stream[-4:])[0]
        if self.interlace:
            self._no("Adam7 interlace")
        elif self.colour_type == 3:
            self._no("palette colour")
        elif self.bit_depth < 8:
            self._no("%d-bit samples" % self.bit_depth)
        elif self.bit_depth == 16 and self.colour_type != 0:
            self._no("16-bit colour")
        elif self.colour_type == 4:
            self._no("gray with alpha")
        if self.H > 65535 or self.W > 65535:
            self._no("size %d x %d above 65535" % (self.H, self.W))
        elif 3 * self.H * self.W >= 1 << 31:
            self._no("3 H W = %d is 2^31 or more" % (3 * self.H * self.W))

    def _require(self):
        if not self.supported:
            raise ValueError("PNG image %s is not supported by the device decoder: %s" % (self.name, self.reason))

    # ---- what the device reads ---------------------------------------------------------------------------------------
    def deflate_bytes(self):
        """the DEFLATE bytes: the zlib stream without its two header bytes and its Adler-32"""
        return self._deflate

    def with_stream(self, deflate, adler=None, name=None):
        """the same header over other DEFLATE bytes (and Adler-32 word), taken as they are: how tests and tools build
        truncated or damaged streams"""
        import copy
        out = copy.copy(self)
        out._deflate = bytes(deflate)
        if adler is not None:
            out.adler = int(adler) & 0xFFFFFFFF
        out.name = name if name is not None else self.name + " (altered)"
        return out

    # ---- the rule in Python / NumPy ----------------------------------------------------------------------------------
    def stream_stats(self):
        """What the DEFLATE stream is made of, by a pure-Python walk (slow; for small files and tests): dict(stored,
        fixed, dynamic: blocks of each type; min_distance, max_distance, max_length: of the matches, 0 without one;
        overlapping: matches with distance < length; max_code_length: the longest Huffman code used; output_bytes;
        status: the status word of the walk, without the size, checksum and filter checks)."""
        status, _, st = inflate_walk(self._deflate, None, keep=False)
        st["status"] = status
        return st

    def inflate_status(self):
        """(status word of stage 1 with its Adler-32 check, the inflated bytes or None): csrc/png_inflate.h in Python"""
        status, out, _ = inflate_walk(self._deflate, self.inflated_bytes)
        if status == 0 and zlib.adler32(out) & 0xFFFFFFFF != self.adler:
            return 8, None
        return status, out

    def parallel_plan(self, chunk_bytes):
        """What ``io_png_decode_par`` does with this stream at ``chunk_bytes``, by the rule of csrc/png_inflate_par.h in
        Python: the contract of the info word and the records.  dict(
        chunks; starts: the candidate bit per chunk, -1 for none; records: per chunk with a candidate dict(exit, exit_bit,
        n, reach, status, next), None otherwise; chain: the chunks the walk from chunk 0 visits; offsets: the output
        offset of each of them; clean; info: the info word; parallel: clean with a chain of two or more;
        symbols: per chain chunk the uint16 symbols (clean images only); resolved: the bytes they resolve to (parallel
        images only, else None); stats: dict(markers: symbols that are markers after the store pass, markers_copied: markers
        that a match copied from inside its chunk, max_reach, reach_chunks: chain chunks in front of it that the longest
        reach spans, stored / fixed / dynamic: blocks decoded by the chain chunks)).  Slow: small files."""
        chunk_bytes = _check_chunk_bytes(chunk_bytes, "parallel_plan")
        data, expected = self._deflate, self.inflated_bytes
        nb = len(data)
        nchunks = (nb + chunk_bytes - 1) // chunk_bytes
        if nchunks > PAR_MAX_CHUNKS:
            raise ValueError("PNG image %s: %d chunks of %d bytes (at most %d)" % (self.name, nchunks, chunk_bytes, PAR_MAX_CHUNKS))
        if getattr(self, "_headers_of", None) is not data:
            self._headers, self._headers_of = np.array(dynamic_header_bits(data), np.int64), data
        chunk_bits = 8 * chunk_bytes
        starts = [-1] * nchunks
        for c in range(nchunks):
            if c == 0:
                starts[c] = 0
                continue
            k = int(np.searchsorted(self._headers, c * chunk_bits))
            if k < self._headers.size and self._headers[k] < min((c + 1) * chunk_bits, 8 * nb):
                starts[c] = int(self._headers[k])
        cands = {s: c for c, s in enumerate(starts) if s >= 0}
        walks = [_chunk_walk(data, s, expected, cands, chunk_bits) if s >= 0 else None for s in starts]
        chain, offsets, clean, off, c = [], [], False, 0, 0
        while c < nchunks:
            r = walks[c]
            chain.append(c)
            offsets.append(off)
            if r["exit"] not in (EXIT_FINAL, EXIT_LINK) or r["reach"] > off or off + r["n"] > expected:
                break
            off += r["n"]
            if r["exit"] == EXIT_FINAL:
                clean = off == expected
                break
            if r["next"] <= c:
                break
            c = r["next"]
        info = min(len(chain), 65535) | (0 if clean else INFO_NOT_CLEAN) | (INFO_CHAIN_OF_ONE if clean and len(chain) < 2 else 0)
        stats = dict(markers=0, markers_copied=0, max_reach=0, reach_chunks=0, stored=0, fixed=0, dynamic=0)
        resolved = None
        if clean:
            for idx, (c, o) in enumerate(zip(chain, offsets)):
                r = walks[c]
                stats["markers"] += sum(1 for v in r["syms"] if v >= 0x8000)
                stats["markers_copied"] += r["copied"]
                for k, name in enumerate(("stored", "fixed", "dynamic")):
                    stats[name] += r["blocks"][k]
                if r["reach"] > stats["max_reach"]:
                    stats["max_reach"] = r["reach"]
                    stats["reach_chunks"] = sum(1 for k in range(idx) if offsets[k + 1] > o - r["reach"])
            if len(chain) >= 2:
                out = bytearray(expected)
                for c, o in zip(chain, offsets):
                    for j, v in enumerate(walks[c]["syms"]):
                        out[o + j] = out[o - 1 - (v & 0x7FFF)] if v >= 0x8000 else v
                resolved = bytes(out)
        keys = ("exit", "exit_bit", "n", "reach", "status", "next")
        return dict(chunks=nchunks, starts=starts, records=[None if w is None else {k: w[k] for k in keys} for w in walks],
                    chain=chain, offsets=offsets, clean=clean, info=info, parallel=clean and len(chain) >= 2,
                    symbols=[np.array(walks[c]["syms"], np.uint16) for c in chain] if clean else None, resolved=resolved,
                    stats=stats)

    def _inflate(self):
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(self._deflate, self.inflated_bytes + 1)
        except zlib.error:
            out = None
        if out is None or not d.eof or len(out) != self.inflated_bytes or zlib.adler32(out) & 0xFFFFFFFF != self.adler:
            status = self.inflate_status()[0]
            raise PngStreamError(status if status else 7, self.name)
        return np.frombuffer(out, np.uint8)

    def to_host(self):
        """uint8 [H, W, 3] (uint16 [H, W] in the raw16 form) by the rule of the module docstring: the contract of the
        kernels.  PngStreamError with the kernel's status word for a stream that does not decode."""
        self._require()
        raw = self._inflate()
        px = _unfilter(raw, self.H, self.rowbytes, self.bpp)
        if px is None:
            raise PngStreamError(9, self.name)
        H, W = self.H, self.W
        if self.raw16:
            return px.reshape(H, W, 2).view(">u2").reshape(H, W).astype(np.uint16)
        if self.channels == 1:
            return np.repeat(px.reshape(H, W, 1), 3, axis=2)
        return np.ascontiguousarray(px.reshape(H, W, self.channels)[:, :, :3])


def is_png(x):
    return isinstance(x, PngImage)


# ---- device side -------------------------------------------------------------------------------------------------------
def descriptors(images, out_offs):
    """(pool uint8, PngDesc array) for a list of supported ``PngImage`` and the byte offset of each decoded image: what
    ``io_png_decode`` reads"""
    desc = (_lib.PngDesc * len(images))()
    chunks, cursor = [], 0
    for k, (im, o) in enumerate(zip(images, out_offs)):
        im._require()
        d = desc[k]
        data = im.deflate_bytes()
        d.data_off, d.data_bytes, d.out_off = cursor, len(data), int(o)
        d.H, d.W, d.channels, d.depth, d.adler = im.H, im.W, im.channels, im.bit_depth, im.adler
        chunks.append(data)
        cursor += len(data)
    pool = np.frombuffer(b"".join(chunks), np.uint8) if cursor else np.zeros(0, np.uint8)
    return pool, desc


DEFAULT_CHUNK_BYTES = 1024
_INFLATE = {"mode": "sequential", "chunk_bytes": DEFAULT_CHUNK_BYTES}


def _check_chunk_bytes(chunk_bytes, who):
    if isinstance(chunk_bytes, bool) or not isinstance(chunk_bytes, (int, np.integer)) or \
            not PAR_MIN_CHUNK <= chunk_bytes <= PAR_MAX_CHUNK or chunk_bytes % PAR_MIN_CHUNK:
        raise ValueError("png.%s: chunk_bytes %r (a multiple of %d in %d..%d)" % (who, chunk_bytes, PAR_MIN_CHUNK, PAR_MIN_CHUNK,
                                                                                  PAR_MAX_CHUNK))
    return int(chunk_bytes)


def set_inflate(mode, chunk_bytes=DEFAULT_CHUNK_BYTES):
    """The inflate stage ``decode``, ``workspace_bytes`` / ``group`` and with them ``PairRenderer`` and ``dense_eval`` use:
    "sequential" -- one wave per image (``io_png_decode``) -- or "parallel" -- one stream on many waves from found block
    starts (``io_png_decode_par``, csrc/png_inflate_par.h), chunks of ``chunk_bytes``.  Bytes and status words do not
    depend on it.  Module-wide; the default is "sequential", the environment variable IO_PNG_INFLATE=parallel selects the
    other at import."""
    if mode not in ("sequential", "parallel"):
        raise ValueError("png.set_inflate: mode %r ('sequential' or 'parallel')" % (mode,))
    _INFLATE.update(mode=mode, chunk_bytes=_check_chunk_bytes(chunk_bytes, "set_inflate"))


def get_inflate(inflate=None):
    """a copy of the setting; ``inflate``: "sequential" / "parallel" instead of the module-wide mode, or a dict to pass on"""
    if isinstance(inflate, dict):
        return dict(inflate)
    s = dict(_INFLATE)
    if inflate is not None:
        if inflate not in ("sequential", "parallel"):
            raise ValueError("png: inflate %r ('sequential' or 'parallel')" % (inflate,))
        s["mode"] = inflate
    return s


if os.environ.get("IO_PNG_INFLATE", ""):
    set_inflate(os.environ["IO_PNG_INFLATE"])


def workspace_bytes(desc, inflate=None):
    s = get_inflate(inflate)
    if s["mode"] == "parallel":
        fn = "io_png_par_workspace_bytes"
        b = int(_lib.lib().io_png_par_workspace_bytes(C.cast(desc, C.c_void_p), len(desc), s["chunk_bytes"]))
    else:
        fn = "io_png_workspace_bytes"
        b = int(_lib.lib().io_png_workspace_bytes(C.cast(desc, C.c_void_p), len(desc)))
    if b == 0:
        raise RuntimeError("instaorder_hip %s refused the descriptors: %s" % (fn, _lib.last_error()))
    return b


def group(images, inflate=None):
    """``arena.Group`` of the PNG files ``images``: blobs (pool, PngDesc array), one ``io_png_decode`` or
    ``io_png_decode_par`` call as ``inflate`` (a mode, a ``get_inflate`` dict, None: the ``set_inflate`` setting) says --
    the same setting sizes the workspace -- and a status word per image; ``info``: the address of int32 info words per
    image (parallel only) or None."""
    if not images:
        return arena.Group()
    s = get_inflate(inflate)
    pool, desc = descriptors(images, [0] * len(images))

    def launch(addrs, out, out_bytes, ws, ws_bytes, status, stream, info=None):
        head = (C.c_void_p(addrs[0]), C.c_size_t(pool.size), C.c_void_p(addrs[1]), C.cast(desc, C.c_void_p), len(desc),
                C.c_void_p(out), C.c_size_t(out_bytes), C.c_void_p(ws), C.c_size_t(ws_bytes), C.c_void_p(status))
        if s["mode"] == "parallel":
            rc = _lib.lib().io_png_decode_par(*(head + (s["chunk_bytes"], C.c_void_p(info), C.c_void_p(stream))))
            _lib.check(rc, "io_png_decode_par")
        else:
            if info is not None:
                raise ValueError("png.group: info words exist with the parallel inflate stage only")
            rc = _lib.lib().io_png_decode(*(head + (C.c_void_p(stream),)))
            _lib.check(rc, "io_png_decode")

    return arena.Group([pool, arena.as_bytes(desc)], ("images", "descriptors"), desc, launch,
                       lambda: workspace_bytes(desc, s), images, raise_for_status)


def raise_for_status(status, images):
    """RuntimeError naming the images whose status word is not zero"""
    bad = [(im.name, int(s)) for im, s in zip(images, status) if int(s) != 0]
    if bad:
        raise RuntimeError("PNG decode failed: " + "; ".join("%s: %s (status %d)" % (nm, STATUS.get(s, "?"), s)
                                                              for nm, s in bad))


def decode(images, device, out=None, check=True, inflate=None, info=False):
    """list of supported ``PngImage`` -> list of device tensors, uint8 [H, W, 3] or uint16 [H, W] (raw16), through one
    ``io_png_decode`` call on the current stream: views of ``out``, a contiguous uint8 device tensor of at least the
    summed sizes (each rounded up to 16 bytes), when given.  Waits for the status words and raises RuntimeError naming
    the images that did not decode; with ``check=False`` it does not wait and returns (tensors, status tensor, images)
    for ``raise_for_status`` later.  A uint16 result may be viewed as int16 storage (``t.view(torch.int16)``), which is
    how ``ext_ops.depth_errors_median`` takes its ground truth.  ``inflate``: "sequential" or "parallel" instead of the
    ``set_inflate`` mode.  With ``info`` (parallel only) the int32 info words of ``io_png_decode_par`` follow the result as
    a NumPy array (a device tensor with ``check=False``)."""
    import torch
    setting = get_inflate(inflate)
    if info and setting["mode"] != "parallel":
        raise ValueError("png.decode: info words exist with the parallel inflate stage only")
    _lib.require_gpu()
    device = torch.device(device)
    images = list(images)
    if not images:
        if info:
            return ([], np.zeros(0, np.int32)) if check else ([], None, [], None)
        return [] if check else ([], None, [])
    for im in images:
        if not is_png(im):
            raise TypeError("png.decode takes PngImage objects (got %s)" % type(im).__name__)
        im._require()
    sizes = [im.out_bytes for im in images]
    lay = arena.Layout()
    offs = [lay.add(s) for s in sizes]
    total = offs[-1] + sizes[-1]
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() < total:
        raise ValueError("png.decode: out must be a contiguous uint8 device tensor of at least %d bytes" % total)
    out = out.view(-1)
    g = group(images, setting)
    g.set_outs(offs)
    status = torch.empty(len(images), dtype=torch.int32, device=out.device)
    words = torch.empty(len(images), dtype=torch.int32, device=out.device) if info else None
    arena.decode_into([g], out, status, words)
    res = []
    for o, s, im in zip(offs, sizes, images):
        t = out[o:o + s]
        res.append(t.view(torch.uint16).view(im.H, im.W) if im.raw16 else t.view(im.H, im.W, 3))
    if not check:
        return (res, status, images, words) if info else (res, status, images)
    raise_for_status(status.cpu().numpy(), images)
    return (res, words.cpu().numpy()) if info else res


def _pil_rgb(path):
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("png.loader: %s is not a file the device decoders take and the default fallback needs "
                           "Pillow, which is not installed; pass fallback=" % path)
    return np.array(Image.open(path).convert("RGB"))


def loader(image_root, jpeg=True, fallback=None, progressive=None):
    """``load_image(image_fn)`` for the dataset classes: a ``PngImage`` for a PNG file in a supported 8-bit form, with
    ``jpeg`` a ``jpeg.JpegImage`` for a JPEG file the device decodes (``progressive`` as in ``jpeg.loader``), otherwise
    ``fallback(path)`` -- by default the reference's own ``np.array(Image.open(path).convert('RGB'))``."""
    fallback = _pil_rgb if fallback is None else fallback

    def load_image(image_fn):
        path = os.path.join(image_root, image_fn)
        with open(path, "rb") as f:
            data = f.read()
        im = None
        try:
            if data[:8] == SIGNATURE:
                im = PngImage(data, name=str(image_fn))
                if im.raw16:
                    im = None
            elif jpeg and data[:2] == b"\xff\xd8":
                from .jpeg import JpegImage
                im = JpegImage(data, name=str(image_fn), progressive=progressive)
        except ValueError:
            im = None
        if im is not None and im.supported:
            return im
        return fallback(path)

    return load_image
