"""Baseline JPEG images for the device input pipeline.

The reference loads an image with ``Image.open(fn).convert('RGB')`` (datasets/occ_order_dataset.py:66-79) and the decoded
H x W x 3 array is what used to travel to the GPU.  A ``JpegImage`` keeps the file's bytes instead: the markers are parsed
here (pure Python, no GPU needed), only the entropy-coded segment, the tables and a descriptor are uploaded -- 5 to 8 times
fewer bytes than the pixels -- and ``io_jpeg_decode_u8`` (csrc/jpeg.hip) decodes in front of the render kernel
(``datasets.PairRenderer``), next to the run-length and polygon masks.

The rule (DESIGN.md "JPEG images") is the published baseline algorithm with libjpeg's default choices; every step is
32-bit two's complement integer arithmetic, there is no floating point:

1. Coefficients: Huffman decode per ITU T.81 F.2.2, DC prediction reset at each restart marker; a coefficient is kept as
   int16 and multiplied by its quantisation table entry, placed through the zig-zag order.
2. IDCT (jidctint.c "islow"): CONST_BITS 13, PASS1_BITS 2; columns first, descaled by 11 with rounding, then rows, descaled
   by 18 with rounding, plus 128, clamped to 0..255.
3. Component planes have ceil(H v / vmax) x ceil(W h / hmax) real samples (stored padded to whole MCUs).
4. Chroma upsampling over the REAL samples (indices clamped at the ends): 4:2:2 ``out[2c] = (3 s[c] + s[c-1] + 1) >> 2``,
   ``out[2c+1] = (3 s[c] + s[c+1] + 2) >> 2``; 4:2:0 first ``t[c] = 3 near[c] + far[c]`` (far = the row above for the upper
   output row, below for the lower one), then ``out[2c] = (3 t[c] + t[c-1] + 8) >> 4``, ``out[2c+1] = (3 t[c] + t[c+1] + 7) >> 4``.
   A chroma plane of at most two real samples per row is replicated instead (libjpeg filters only wider planes).
5. Colour with cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
   G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), arithmetic shifts, clamped to 0..255.  Grayscale: R = G = B = Y.

``JpegImage.to_host()`` is that rule in NumPy and the contract of the kernels.  Equality with libjpeg-turbo is claimed for
streams whose dequantised coefficients fit int16 (its SIMD path holds them in 16 bits).  EXIF orientation is ignored, as
``convert('RGB')`` ignores it.
"""
import ctypes as C
import os
import re
import struct

import numpy as np

from . import _lib

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63])
LOOKUP_BITS = 8              # JPEG_LOOKUP_BITS of csrc/jpeg_entropy.h
STATUS = {1: "bits that are no Huffman code", 2: "a zero run past coefficient 63", 3: "a restart marker missing or out of order",
          4: "entropy-coded data exhausted", 5: "a DC category above 15"}
TABLES_BYTES = 1600          # sizeof(io_jpeg_tables)

_SOF_REASON = {0xC1: "extended sequential DCT", 0xC2: "progressive DCT", 0xC3: "lossless", 0xC5: "differential sequential DCT",
               0xC6: "differential progressive DCT", 0xC7: "differential lossless", 0xC9: "arithmetic coding",
               0xCA: "arithmetic coding (progressive)", 0xCB: "arithmetic coding (lossless)", 0xCD: "arithmetic coding",
               0xCE: "arithmetic coding", 0xCF: "arithmetic coding"}
_FILL = re.compile(rb"\xff+(?=\xff)")
_RST = re.compile(rb"\xff[\xd0-\xd7]")
_MARKER = re.compile(rb"\xff(?:[^\x00]|$)")


class JpegStreamError(ValueError):
    """the entropy-coded data of a well-formed file does not decode; ``status`` is the kernel's status word"""

    def __init__(self, status, name):
        ValueError.__init__(self, "JPEG image %s: %s (status %d)" % (name, STATUS.get(status, "?"), status))
        self.status = status


def _u16(b, p):
    return struct.unpack_from(">H", b, p)[0]


class JpegImage(object):
    """One JPEG file, parsed but not decoded.  Stands in for a uint8 [H, W, 3] array where the consumers only look at
    ``shape`` / ``dtype``; ``supported`` says whether the device decoder takes it (``reason`` why not)."""
    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, data, name=None):
        self.data = bytes(data)
        self.name = name if name is not None else "<%d bytes>" % len(self.data)
        self.reason = None
        self.H = self.W = 0
        self.components = []            # (id, h, v, quant table) in frame order
        self.restart_interval = 0
        self.entropy = (0, 0)           # [start, end) of the entropy-coded segment in data
        self._tables = None
        self._entropy = None
        self._parse()

    @classmethod
    def open(cls, path):
        with open(path, "rb") as f:
            return cls(f.read(), name=str(path))

    # ---- the array surface -------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return (self.H, self.W, 3)

    @property
    def supported(self):
        return self.reason is None

    @property
    def nbytes_compressed(self):
        return len(self.data)

    @property
    def nbytes_entropy(self):
        return self.entropy[1] - self.entropy[0]

    def _no(self, reason):
        if self.reason is None:
            self.reason = reason

    # ---- markers -----------------------------------------------------------------------------------------------------
    def _parse(self):
        b = self.data
        n = len(b)
        if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
            raise ValueError("JPEG %s: no SOI marker" % self.name)
        p = 2
        quant, huff = {}, {}
        jfif, adobe = False, None
        sof = None
        scans = 0
        scan_sel = None
        while True:
            if p >= n:
                raise ValueError("JPEG %s: the file ends without an EOI marker" % self.name)
            if b[p] != 0xFF:
                raise ValueError("JPEG %s: byte %d is 0x%02x where a marker was expected" % (self.name, p, b[p]))
            while p < n and b[p] == 0xFF:                    # fill bytes
                p += 1
            if p >= n:
                raise ValueError("JPEG %s: the file ends inside a marker" % self.name)
            m = b[p]
            p += 1
            if m == 0xD9:                                    # EOI; what follows is ignored
                break
            if m == 0x00:
                raise ValueError("JPEG %s: a stuffed FF 00 outside entropy-coded data (byte %d)" % (self.name, p - 2))
            if m == 0x01 or 0xD0 <= m <= 0xD7:
                continue
            if m == 0xD8:
                raise ValueError("JPEG %s: a second SOI marker" % self.name)
            if p + 2 > n:
                raise ValueError("JPEG %s: the file ends inside a segment header" % self.name)
            L = _u16(b, p)
            if L < 2 or p + L > n:
                raise ValueError("JPEG %s: segment 0x%02x of length %d runs past the end of the file" % (self.name, m, L))
            s = b[p + 2:p + L]
            p += L
            if m == 0xE0 and s[:5] == b"JFIF\0":
                jfif = True
            elif m == 0xEE and s[:5] == b"Adobe" and len(s) >= 12:
                adobe = s[11]
            elif m == 0xDB:
                i = 0
                while i < len(s):
                    pq, tq = s[i] >> 4, s[i] & 15
                    size = 64 * (2 if pq else 1)
                    if pq > 1 or tq > 3 or i + 1 + size > len(s):
                        raise ValueError("JPEG %s: malformed DQT segment" % self.name)
                    quant[tq] = None if pq else np.frombuffer(s, np.uint8, 64, i + 1).astype(np.uint16)
                    i += 1 + size
            elif m == 0xC4:
                i = 0
                while i < len(s):
                    if i + 17 > len(s):
                        raise ValueError("JPEG %s: malformed DHT segment" % self.name)
                    tc, th = s[i] >> 4, s[i] & 15
                    counts = np.frombuffer(s, np.uint8, 16, i + 1)
                    k = int(counts.sum())
                    if tc > 1 or th > 3 or k > 256 or i + 17 + k > len(s):
                        raise ValueError("JPEG %s: malformed DHT segment" % self.name)
                    huff[(tc, th)] = (counts.copy(), np.frombuffer(s, np.uint8, k, i + 17).copy())
                    i += 17 + k
            elif m == 0xDD:
                if len(s) < 2:
                    raise ValueError("JPEG %s: malformed DRI segment" % self.name)
                self.restart_interval = _u16(s, 0)
            elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
                if sof is not None:
                    raise ValueError("JPEG %s: a second frame header" % self.name)
                if len(s) < 6 or len(s) < 6 + 3 * s[5]:
                    raise ValueError("JPEG %s: malformed frame header" % self.name)
                sof = m
                precision, self.H, self.W = s[0], _u16(s, 1), _u16(s, 3)
                self.components = [(s[6 + 3 * k], s[7 + 3 * k] >> 4, s[7 + 3 * k] & 15, s[8 + 3 * k]) for k in range(s[5])]
                if m != 0xC0:
                    self._no("not baseline: " + _SOF_REASON.get(m, "frame type 0x%02x" % m))
                elif precision != 8:
                    self._no("%d-bit samples" % precision)
                if self.H == 0 or self.W == 0:
                    self._no("zero dimension (%d x %d)" % (self.H, self.W))
            elif m == 0xCC:
                self._no("arithmetic coding")
            elif m == 0xDA:
                if sof is None:
                    raise ValueError("JPEG %s: a scan in front of the frame header" % self.name)
                if len(s) < 1 or len(s) < 4 + 2 * s[0]:
                    raise ValueError("JPEG %s: malformed scan header" % self.name)
                scans += 1
                start = q = p
                while True:                                  # the entropy-coded segment ends at the next real marker
                    q = b.find(b"\xff", q)
                    if q < 0 or q + 1 >= n:
                        raise ValueError("JPEG %s: the file ends without an EOI marker" % self.name)
                    if b[q + 1] == 0x00 or 0xD0 <= b[q + 1] <= 0xD7:
                        q += 2
                    elif b[q + 1] == 0xFF:
                        q += 1
                    else:
                        break
                if scans == 1:
                    ns = s[0]
                    scan_sel = ([(s[1 + 2 * k], s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15) for k in range(ns)],
                                tuple(s[1 + 2 * ns:4 + 2 * ns]))
                    self.entropy = (start, q)
                    self._tables = (dict(quant), dict(huff))     # the tables in effect at the scan
                p = q
        if sof is None or scans == 0:
            raise ValueError("JPEG %s: no frame or no scan" % self.name)
        if scans > 1:
            self._no("%d scans" % scans)
        self._classify(scan_sel, jfif, adobe)

    def _classify(self, scan_sel, jfif, adobe):
        comps = self.components
        sel, (ss, se, ahal) = scan_sel
        if len(comps) not in (1, 3):
            self._no("%d components (CMYK / YCCK)" % len(comps) if len(comps) == 4 else "%d components" % len(comps))
            return
        if [c[0] for c in comps] != [c[0] for c in sel]:
            self._no("the scan does not interleave all components in frame order")
            return
        if (ss, se, ahal) != (0, 63, 0):
            self._no("spectral selection / successive approximation in a sequential scan")
            return
        if len(comps) == 3:
            ids = bytes(c[0] for c in comps)
            if not (jfif or (adobe is None and ids != b"RGB") or adobe == 1):
                self._no("RGB colour space (Adobe transform %s)" % adobe)
                return
            samp = tuple((c[1], c[2]) for c in comps)
            if samp[1:] != ((1, 1), (1, 1)) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
                self._no("sampling %s" % " ".join("%dx%d" % hv for hv in samp))
                return
        elif (comps[0][1], comps[0][2]) != (1, 1):
            self._no("sampling %dx%d of a single component" % (comps[0][1], comps[0][2]))
            return
        quant, huff = self._tables
        for (cid, h, v, tq), (_, td, ta) in zip(comps, sel):
            if tq not in quant:
                self._no("quantisation table %d is missing" % tq)
            elif quant[tq] is None:
                self._no("16-bit quantisation table")
            if td > 1 or ta > 1:
                self._no("Huffman table id above 1 in a baseline file")
            elif (0, td) not in huff or (1, ta) not in huff:
                self._no("a Huffman table is missing")
        self.scan_tables = [(td, ta) for _, td, ta in sel]

    # ---- what the device reads ---------------------------------------------------------------------------------------
    @property
    def luma_sampling(self):
        return (self.components[0][1], self.components[0][2]) if len(self.components) == 3 else (1, 1)

    def entropy_bytes(self):
        if self._entropy is not None:
            return self._entropy
        return self.data[self.entropy[0]:self.entropy[1]]

    def with_entropy(self, data, name=None):
        """the same headers over other entropy-coded bytes, taken as they are (nothing is parsed again): how tests and
        tools build truncated or damaged streams"""
        import copy
        out = copy.copy(self)
        out._entropy = bytes(data)
        out.name = name if name is not None else self.name + " (altered)"
        return out

    def tables_blob(self):
        """the io_jpeg_tables record of this file (bytes): equal for files that share their tables"""
        self._require()
        quant, huff = self._tables
        rec = np.zeros(TABLES_BYTES, np.uint8)
        q16 = rec[:512].view(np.uint16).reshape(4, 64)
        counts = rec[512:576].reshape(4, 16)
        syms = rec[576:].reshape(4, 256)
        for tq, tab in quant.items():
            if tab is not None:
                q16[tq] = tab
        for (tc, th), (cnt, sy) in huff.items():
            if th < 2:
                counts[2 * tc + th] = cnt
                syms[2 * tc + th, :len(sy)] = sy
        return rec.tobytes()

    def _require(self):
        if not self.supported:
            raise ValueError("JPEG image %s is not supported by the device decoder: %s" % (self.name, self.reason))

    # ---- the rule in NumPy -------------------------------------------------------------------------------------------
    def coefficients(self, stats=None):
        """int16 [n_blocks, 64] in decode order, natural order inside a block: stage 1 of the rule (JpegStreamError for a
        stream the kernel would flag).  ``stats``: a dict that receives symbols (Huffman symbols decoded), zrl,
        max_code_length and max_dc_category."""
        self._require()
        st = dict(symbols=0, zrl=0, max_code_length=0, max_dc_category=0)
        quant, huff = self._tables
        hs, vs = self.luma_sampling
        nc = len(self.components)
        mw, mh = -(-self.W // (8 * hs)), -(-self.H // (8 * vs))
        luma = hs * vs
        bpm = luma + (2 if nc == 3 else 0)
        looks = {}
        for key, (cnt, sy) in huff.items():                  # 16-bit prefix -> (length, symbol); length 0: no code
            ln = np.zeros(1 << 16, np.uint8)
            sv = np.zeros(1 << 16, np.uint8)
            code, k, ok = 0, 0, True
            for l in range(1, 17):
                for _ in range(int(cnt[l - 1])):
                    if code >= 1 << l:
                        ok = False
                        break
                    lo = code << (16 - l)
                    ln[lo:lo + (1 << (16 - l))] = l
                    sv[lo:lo + (1 << (16 - l))] = sy[k]
                    code += 1
                    k += 1
                code <<= 1
            if not ok:
                raise ValueError("JPEG %s: Huffman code lengths that form no prefix code" % self.name)
            looks[key] = (ln, sv)
        # FF fill bytes are dropped; split at the restart markers; inside an interval the reader stops at any other marker
        raw = _FILL.sub(b"", self.entropy_bytes())
        segs, marks, at = [], [], 0
        for mt in _RST.finditer(raw):
            segs.append(raw[at:mt.start()])
            marks.append(raw[mt.end() - 1] - 0xD0)
            at = mt.end()
        segs.append(raw[at:])
        clean, cut = [], []
        for sg in segs:
            mt = _MARKER.search(sg)
            cut.append(mt is not None)
            if mt:
                sg = sg[:mt.start()]
            clean.append(sg.replace(b"\xff\x00", b"\xff"))
        coef = np.zeros((mw * mh * bpm, 64), np.int16)
        state = dict(seg=0, buf=clean[0] + b"\0" * 8, bits=8 * len(clean[0]), pos=0)

        def peek16():
            p = state["pos"]
            return (int.from_bytes(state["buf"][p >> 3:(p >> 3) + 4], "big") >> (16 - (p & 7))) & 0xFFFF

        def skip(k):
            state["pos"] += k
            if state["pos"] > state["bits"]:
                raise JpegStreamError(4, self.name)

        def symbol(tab):
            c = peek16()
            l = int(tab[0][c])
            if l == 0:
                raise JpegStreamError(1, self.name)
            skip(l)
            st["symbols"] += 1
            st["max_code_length"] = max(st["max_code_length"], l)
            return int(tab[1][c])

        def receive_extend(s):
            v = peek16() >> (16 - s)
            skip(s)
            return v if v >= 1 << (s - 1) else v - (1 << s) + 1

        pred = [0, 0, 0]
        blk = 0
        if stats is not None:
            stats.update(st)
            st = stats
        for mcu in range(mw * mh):
            if self.restart_interval and mcu and mcu % self.restart_interval == 0:
                k = state["seg"]
                if state["bits"] - state["pos"] >= 8 or cut[k] or k >= len(marks) or marks[k] != k % 8:
                    raise JpegStreamError(3, self.name)
                state.update(seg=k + 1, buf=clean[k + 1] + b"\0" * 8, bits=8 * len(clean[k + 1]), pos=0)
                pred = [0, 0, 0]
            for r in range(bpm):
                comp = 0 if r < luma else 1 + r - luma
                td, ta = self.scan_tables[comp]
                t = symbol(looks[(0, td)])
                if t > 15:
                    raise JpegStreamError(5, self.name)
                st["max_dc_category"] = max(st["max_dc_category"], t)
                if t:
                    pred[comp] += receive_extend(t)
                coef[blk, 0] = np.int64(pred[comp]).astype(np.int16)
                k = 1
                while k < 64:
                    rs = symbol(looks[(1, ta)])
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run != 15:
                            break
                        k += 16
                        st["zrl"] += 1
                        if k > 64:
                            raise JpegStreamError(2, self.name)
                        continue
                    k += run
                    if k > 63:
                        raise JpegStreamError(2, self.name)
                    coef[blk, ZIGZAG[k]] = receive_extend(size)
                    k += 1
                blk += 1
        return coef

    def to_host(self):
        """uint8 [H, W, 3] by the rule of the module docstring, in NumPy: the contract of the kernels.  Slow."""
        coef = self.coefficients()
        quant, _ = self._tables
        hs, vs = self.luma_sampling
        nc = len(self.components)
        H, W = self.H, self.W
        mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
        luma = hs * vs
        bpm = luma + (2 if nc == 3 else 0)
        blocks = coef.reshape(mh, mw, bpm, 64)
        planes = []
        for c in range(nc):
            q = np.zeros(64, np.int32)
            q[ZIGZAG] = quant[self.components[c][3]].astype(np.int32)
            if c == 0:
                px = _idct(blocks[:, :, :luma].astype(np.int32) * q)            # [mh, mw, luma, 8, 8]
                px = px.reshape(mh, mw, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * vs * 8, mw * hs * 8)
            else:
                px = _idct(blocks[:, :, luma + c - 1].astype(np.int32) * q)     # [mh, mw, 8, 8]
                px = px.transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8)
            planes.append(px)
        Y = planes[0][:H, :W]
        if nc == 1:
            return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8)
        ch, cw = -(-H // vs), -(-W // hs)
        cb, cr = [_upsample(p[:ch, :cw], hs, vs)[:H, :W] - 128 for p in planes[1:]]
        R = Y + ((91881 * cr + 32768) >> 16)
        G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        B = Y + ((116130 * cb + 32768) >> 16)
        return np.clip(np.stack([R, G, B], 2), 0, 255).astype(np.uint8)


def _idct8(i0, i1, i2, i3, i4, i5, i6, i7):
    """one 8-point pass of jidctint.c on int32 arrays, without the descale"""
    z1 = (i2 + i6) * 4433
    t2 = z1 + i6 * (-15137)
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) * 8192
    t1 = (i0 - i4) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * (-7373), z2 * (-20995)
    z3 = z3 * (-16069) + z5
    z4 = z4 * (-3196) + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]


def _idct(c):
    """dequantised int32 [..., 64] -> samples int32 [..., 8, 8] in 0..255 (32-bit arithmetic, wrapping as the kernel's)"""
    with np.errstate(over="ignore"):
        c = c.astype(np.int32).reshape(c.shape[:-1] + (8, 8))
        cols = _idct8(*[c[..., r, :] for r in range(8)])                         # over rows r, for every column
        ws = np.stack([(o + np.int32(1 << 10)) >> 11 for o in cols], axis=-2)
        rows = _idct8(*[ws[..., :, x] for x in range(8)])
        out = np.stack([((o + np.int32(1 << 17)) >> 18) + 128 for o in rows], axis=-1)
    return np.clip(out, 0, 255).astype(np.int32)


def _upsample(P, hs, vs):
    """step 4 on one chroma plane of real samples (int32 [ch, cw]) -> [ch * vs, cw * hs]"""
    if hs == 1:
        return P
    if P.shape[1] <= 2:                  # libjpeg filters only planes more than two samples wide
        return np.repeat(np.repeat(P, vs, axis=0), hs, axis=1)
    if vs == 2:
        up = np.concatenate([P[:1], P[:-1]])
        down = np.concatenate([P[1:], P[-1:]])
        T = np.empty((2 * P.shape[0], P.shape[1]), np.int32)
        T[0::2] = 3 * P + up
        T[1::2] = 3 * P + down
        add, shift = (8, 7), 4
    else:
        T = P
        add, shift = (1, 2), 2
    left = np.concatenate([T[:, :1], T[:, :-1]], 1)
    right = np.concatenate([T[:, 1:], T[:, -1:]], 1)
    out = np.empty((T.shape[0], 2 * T.shape[1]), np.int32)
    out[:, 0::2] = (3 * T + left + add[0]) >> shift
    out[:, 1::2] = (3 * T + right + add[1]) >> shift
    return out


def is_jpeg(x):
    return isinstance(x, JpegImage)


# ---- device side -------------------------------------------------------------------------------------------------------
def descriptors(images, out_offs):
    """(pool uint8, tables uint8 [n_sets * 1600], JpegDesc array) for a list of supported ``JpegImage`` and the byte offset
    of each decoded image: what ``io_jpeg_decode_u8`` reads.  Identical table sets are stored once."""
    desc = (_lib.JpegDesc * len(images))()
    sets, blobs, chunks, cursor = {}, [], [], 0
    for k, (im, o) in enumerate(zip(images, out_offs)):
        blob = im.tables_blob()
        if blob not in sets:
            sets[blob] = len(blobs)
            blobs.append(blob)
        d = desc[k]
        ent = im.entropy_bytes()
        d.data_off, d.data_bytes, d.out_off = cursor, len(ent), int(o)
        d.H, d.W, d.n_comp = im.H, im.W, len(im.components)
        d.hs, d.vs = im.luma_sampling
        d.restart_interval, d.table_set = im.restart_interval, sets[blob]
        for c, ((cid, h, v, tq), (td, ta)) in enumerate(zip(im.components, im.scan_tables)):
            d.quant[c], d.dc[c], d.ac[c] = tq, td, ta
        chunks.append(ent)
        cursor += len(ent)
    pool = np.frombuffer(b"".join(chunks), np.uint8) if cursor else np.zeros(0, np.uint8)
    tables = np.frombuffer(b"".join(blobs), np.uint8)
    return pool, tables, desc


def workspace_bytes(desc):
    b = int(_lib.lib().io_jpeg_workspace_bytes(C.cast(desc, C.c_void_p), len(desc)))
    if b == 0:
        raise RuntimeError("instaorder_hip io_jpeg_workspace_bytes refused the descriptors: %s" % _lib.last_error())
    return b


def raise_for_status(status, images):
    """RuntimeError naming the images whose status word is not zero"""
    bad = [(im.name, int(s)) for im, s in zip(images, status) if int(s) != 0]
    if bad:
        raise RuntimeError("JPEG decode failed: " + "; ".join("%s: %s (status %d)" % (nm, STATUS.get(s, "?"), s)
                                                               for nm, s in bad))


def decode(images, device, out=None):
    """list of supported ``JpegImage`` -> list of uint8 [H, W, 3] device tensors through one ``io_jpeg_decode_u8`` call on
    the current stream (views of ``out``, a contiguous uint8 device tensor of at least the summed sizes, when given).
    Waits for the status words and raises RuntimeError naming the images that did not decode."""
    import torch
    _lib.require_gpu()
    device = torch.device(device)
    images = list(images)
    if not images:
        return []
    for im in images:
        if not is_jpeg(im):
            raise TypeError("jpeg.decode takes JpegImage objects (got %s)" % type(im).__name__)
        im._require()
    sizes = [im.H * im.W * 3 for im in images]
    offs = [0]
    for s in sizes[:-1]:
        offs.append(offs[-1] + (s + 15) // 16 * 16)
    total = offs[-1] + sizes[-1]
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() < total:
        raise ValueError("jpeg.decode: out must be a contiguous uint8 device tensor of at least %d bytes" % total)
    out = out.view(-1)
    pool, tables, desc = descriptors(images, offs)
    blobs = [tables, np.frombuffer(desc, dtype=np.uint8), pool]
    at, cursor = [], 0
    for b in blobs:
        at.append(cursor)
        cursor += (b.size + 15) // 16 * 16
    host = np.zeros(max(cursor, 16), np.uint8)
    for a, b in zip(at, blobs):
        host[a:a + b.size] = b
    dev = torch.from_numpy(host).to(out.device)
    ws = torch.empty(workspace_bytes(desc), dtype=torch.uint8, device=out.device)
    status = torch.empty(len(images), dtype=torch.int32, device=out.device)
    base = dev.data_ptr()
    rc = _lib.lib().io_jpeg_decode_u8(
        C.c_void_p(base + at[2]), C.c_size_t(pool.size), C.c_void_p(base + at[0]), tables.ctypes.data_as(C.c_void_p),
        C.c_size_t(tables.size), C.c_void_p(base + at[1]), C.cast(desc, C.c_void_p), len(images), C.c_void_p(out.data_ptr()),
        C.c_size_t(out.numel()), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel()), C.c_void_p(status.data_ptr()),
        C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream))
    _lib.check(rc, "io_jpeg_decode_u8")
    raise_for_status(status.cpu().numpy(), images)
    return [out[o:o + s].view(im.H, im.W, 3) for o, s, im in zip(offs, sizes, images)]


def _pil_rgb(path):
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("jpeg.loader: %s is not a JPEG file the device decoder takes and the default fallback needs "
                           "Pillow, which is not installed; pass fallback=" % path)
    return np.array(Image.open(path).convert("RGB"))


def loader(image_root, fallback=None):
    """``load_image(image_fn)`` for the dataset classes: a ``JpegImage`` for a file the device decodes, otherwise
    ``fallback(path)`` -- by default the reference's own ``np.array(Image.open(path).convert('RGB'))``."""
    fallback = _pil_rgb if fallback is None else fallback

    def load_image(image_fn):
        path = os.path.join(image_root, image_fn)
        with open(path, "rb") as f:
            data = f.read()
        if data[:2] == b"\xff\xd8":
            try:
                im = JpegImage(data, name=str(image_fn))
            except ValueError:
                im = None
            if im is not None and im.supported:
                return im
        return fallback(path)

    return load_image
