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

Step 1 has two implementations on the device with the same result: one lane per image (``io_jpeg_decode_u8``, the default)
and the lanes of a workgroup on the subsequences of one image (``io_jpeg_decode_par_u8``, csrc/jpeg_sync.h), chosen by
``set_entropy``; ``JpegImage.parallel_plan`` is the rule of the latter in Python.

Progressive files (SOF2) are refused by default ("not baseline: progressive DCT") and go to the loader's fallback.  With
``set_progressive("device")``, ``JpegImage(..., progressive=True)`` or IO_JPEG_PROGRESSIVE=device the complete progressions of
DESIGN.md "Progressive JPEG" are accepted: step 1 then fills the same coefficients over the file's scans by T.81 G.1.2
(``JpegImage.scans``, ``scan_levels``; ``io_jpeg_decode_prog_u8``, csrc/jpeg_prog.h), steps 2 to 5 are unchanged.
"""
import collections
import ctypes as C
import os
import re
import struct

import numpy as np

from . import _lib, arena

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


# one scan of an accepted progressive file: component indices in frame order, Ss, Se, Ah, Al, [start, end) of its
# entropy-coded segment in the file, the restart interval in effect, and per scan component the (16 counts, symbols) bytes of
# the Huffman table in effect -- the DC table in a DC scan, the AC table in an AC scan, None in a DC refinement
ProgScan = collections.namedtuple("ProgScan", "comps ss se ah al start end restart_interval tables")


class JpegImage(object):
    """One JPEG file, parsed but not decoded.  Stands in for a uint8 [H, W, 3] array where the consumers only look at
    ``shape`` / ``dtype``; ``supported`` says whether the device decoder takes it (``reason`` why not)."""
    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, data, name=None, progressive=None):
        self.data = bytes(data)
        self.name = name if name is not None else "<%d bytes>" % len(self.data)
        self.reason = None
        self.progressive = False        # an accepted SOF2 file: ``scans`` holds its scans
        self.scans = []
        self._scan_data = {}
        self._want_progressive = (get_progressive() == "device") if progressive is None else bool(progressive)
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
        prog, late_dqt = [], False      # every scan as (selectors, Ss, Se, Ah, Al, start, end, DRI, Huffman tables) in file order
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
                late_dqt = late_dqt or scans > 0
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
                if m != 0xC0 and not (m == 0xC2 and self._want_progressive):
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
                ns = s[0]
                prog.append(([(s[1 + 2 * k], s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15) for k in range(ns)], s[1 + 2 * ns],
                             s[2 + 2 * ns], s[3 + 2 * ns] >> 4, s[3 + 2 * ns] & 15, start, q, self.restart_interval, dict(huff)))
                if scans == 1:
                    scan_sel = ([(s[1 + 2 * k], s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15) for k in range(ns)],
                                tuple(s[1 + 2 * ns:4 + 2 * ns]))
                    self.entropy = (start, q)
                    self._tables = (dict(quant), dict(huff))     # the tables in effect at the scan
                p = q
        if sof is None or scans == 0:
            raise ValueError("JPEG %s: no frame or no scan" % self.name)
        if sof == 0xC2 and self._want_progressive:
            self._tables = (self._tables[0], {})
            if self.reason is None:
                self._classify_progressive(prog, late_dqt, jfif, adobe)
            return
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
        if not self._classify_frame(jfif, adobe):
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

    def _classify_frame(self, jfif, adobe):
        """the colour-space and sampling rules, the same for baseline and progressive files"""
        comps = self.components
        if len(comps) == 3:
            ids = bytes(c[0] for c in comps)
            if not (jfif or (adobe is None and ids != b"RGB") or adobe == 1):
                self._no("RGB colour space (Adobe transform %s)" % adobe)
                return False
            samp = tuple((c[1], c[2]) for c in comps)
            if samp[1:] != ((1, 1), (1, 1)) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
                self._no("sampling %s" % " ".join("%dx%d" % hv for hv in samp))
                return False
        elif (comps[0][1], comps[0][2]) != (1, 1):
            self._no("sampling %dx%d of a single component" % (comps[0][1], comps[0][2]))
            return False
        return True

    def _classify_progressive(self, prog, late_dqt, jfif, adobe):
        """the rules of DESIGN.md "Progressive JPEG": which SOF2 files the device takes; fills ``scans``"""
        comps = self.components
        why = "progressive DCT: "
        if len(comps) not in (1, 3):
            return self._no(why + ("%d components (CMYK / YCCK)" % len(comps) if len(comps) == 4 else "%d components" % len(comps)))
        if not self._classify_frame(jfif, adobe):
            self.reason = why + self.reason
            return
        if late_dqt:
            return self._no(why + "a quantisation table defined between scans")
        quant = self._tables[0]
        for cid, h, v, tq in comps:
            if tq not in quant:
                return self._no(why + "quantisation table %d is missing" % tq)
            if quant[tq] is None:
                return self._no(why + "16-bit quantisation table")
        index = {c[0]: k for k, c in enumerate(comps)}
        al_of = [[None] * 64 for _ in comps]                 # the Al every coefficient has been sent down to
        out = []
        for n, (sel, ss, se, ah, al, start, end, ri, huff) in enumerate(prog):
            what = why + "scan %d " % n
            cs = [index.get(cid, -1) for cid, td, ta in sel]
            if not cs or min(cs) < 0 or cs != sorted(set(cs)):
                return self._no(what + "does not name components of the frame in frame order")
            if ss == 0:
                if se != 0:
                    return self._no(what + "mixes DC and AC coefficients (Ss 0, Se %d)" % se)
                if len(cs) != 1 and len(cs) != len(comps):
                    return self._no(what + "is a DC scan of %d of %d components" % (len(cs), len(comps)))
            elif len(cs) != 1 or not 1 <= ss <= se <= 63:
                return self._no(what + "is an AC scan of %d components with Ss %d, Se %d" % (len(cs), ss, se))
            if al > 13:
                return self._no(what + "has Al %d above 13" % al)
            if ah != 0 and ah != al + 1:
                return self._no(what + "refines by more than one bit (Ah %d, Al %d)" % (ah, al))
            tabs = []
            for c, (cid, td, ta) in zip(cs, sel):
                if ss and al_of[c][0] is None:
                    return self._no(what + "is an AC scan in front of the DC scan of its component")
                have = set(al_of[c][ss:se + 1])
                if ah == 0 and have != {None}:
                    return self._no(what + "sends coefficients a second time")
                if ah and have != {ah}:
                    return self._no(what + "refines coefficients that are not at Al %d" % ah)
                al_of[c][ss:se + 1] = [al] * (se + 1 - ss)
                key = (1, ta) if ss else (0, td)
                if ss == 0 and ah:
                    tabs.append(None)                        # a DC refinement reads plain bits
                elif key not in huff:
                    return self._no(what + "names a Huffman table that is missing")
                else:
                    tabs.append((huff[key][0].tobytes(), huff[key][1].tobytes()))
            out.append(ProgScan(tuple(cs), ss, se, ah, al, start, end, ri, tuple(tabs)))
        for c in range(len(comps)):
            if al_of[c][0] is None:
                return self._no(why + "incomplete progression: no DC scan of component %d" % c)
            if any(a != 0 for a in al_of[c]):
                k = [a != 0 for a in al_of[c]].index(True)
                return self._no(why + "incomplete progression: coefficient %d of component %d %s" % (
                    k, c, "is never sent" if al_of[c][k] is None else "stops at Al %d" % al_of[c][k]))
        self.scans = out
        self.progressive = True
        self.restart_interval = out[0].restart_interval
        self.entropy = (out[0].start, out[-1].end)

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
        if self.progressive:
            return self._coefficients_progressive(stats)
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

    # ---- progressive files: the scans, their levels and the rule of csrc/jpeg_prog.h in Python ------------------------------
    def scan_bytes(self, index):
        """the entropy-coded segment of scan ``index`` of a progressive file"""
        if index in self._scan_data:
            return self._scan_data[index]
        return self.data[self.scans[index].start:self.scans[index].end]

    def with_scan(self, index, data, name=None):
        """``with_entropy`` for one scan of a progressive file"""
        import copy
        out = copy.copy(self)
        out._scan_data = dict(self._scan_data)
        out._scan_data[index] = bytes(data)
        out.name = name if name is not None else self.name + " (scan %d altered)" % index
        return out

    def scan_levels(self):
        """per scan: 1 + the highest level of an earlier scan that shares a (component, coefficient) pair with it, 0 if
        there is none; an AC scan counts the first DC scan of its component among them, as the format orders the two (so
        the levels follow the file's own order of dependence: Pillow's ten-scan colour script has four).  Scans of one
        level touch disjoint coefficients, so the device runs them side by side."""
        last, first_dc, levels = {}, {}, []
        for sc in self.scans:
            pairs = [(c, k) for c in sc.comps for k in range(sc.ss, sc.se + 1)]
            lv = 1 + max([last.get(p, -1) for p in pairs] + [first_dc.get(c, -1) for c in sc.comps if sc.ss])
            for p in pairs:
                last[p] = lv
            if sc.ss == 0:
                for c in sc.comps:
                    first_dc.setdefault(c, lv)
            levels.append(lv)
        return levels

    def scan_blocks(self, index):
        """(block index in the [n_blocks, 64] MCU-ordered buffer of every block of the scan in scan order, blocks per MCU
        of the scan, blocks across, blocks down).  A scan of all components walks the MCUs; a scan of one component walks
        that component's own ceil(w_c / 8) x ceil(h_c / 8) raster, an MCU being one block."""
        sc = self.scans[index]
        hs, vs = self.luma_sampling
        nc = len(self.components)
        mw, mh = -(-self.W // (8 * hs)), -(-self.H // (8 * vs))
        luma = hs * vs
        bpm = luma + (2 if nc == 3 else 0)
        if len(sc.comps) > 1:
            return np.arange(mw * mh * bpm), bpm, mw, mh
        c = sc.comps[0]
        ch, cv = (hs, vs) if c == 0 else (1, 1)
        bw = -(-(-(-self.W * ch // hs)) // 8)
        bh = -(-(-(-self.H * cv // vs)) // 8)
        by, bx = np.mgrid[0:bh, 0:bw]
        r = (by % cv) * ch + bx % ch if c == 0 else luma + c - 1
        return (((by // cv) * mw + bx // ch) * bpm + r).reshape(-1), 1, bw, bh

    def _coefficients_progressive(self, stats):
        st = dict(symbols=0, zrl=0, max_code_length=0, max_dc_category=0, eobrun_max=0, eobrun_refine_max=0, zrl_refine=0,
                  correction_bits=0, restarts=0)
        if stats is not None:
            stats.update(st)
            st = stats
        hs, vs = self.luma_sampling
        mw, mh = -(-self.W // (8 * hs)), -(-self.H // (8 * vs))
        bpm = hs * vs + (2 if len(self.components) == 3 else 0)
        coef = np.zeros((mw * mh * bpm, 64), np.int64)
        for n in range(len(self.scans)):
            self._decode_scan(n, coef, st)
        return coef.astype(np.int16)

    def _decode_scan(self, index, coef, st):
        """one scan by T.81 G.1.2 into ``coef`` (int64 [n_blocks, 64] holding int16 values)"""
        sc = self.scans[index]
        ss, se, ah, al = sc.ss, sc.se, sc.ah, sc.al
        order, per_mcu, _, _ = self.scan_blocks(index)
        luma = self.luma_sampling[0] * self.luma_sampling[1]
        looks = [None if t is None else _lookup(t[0], t[1], self.name) for t in sc.tables]
        bits = _Bits(self.scan_bytes(index), self.name)
        zz = [int(v) for v in ZIGZAG]
        p1, m1 = 1 << al, -1 << al

        def symbol(tab):
            c = bits.peek16()
            l = int(tab[0][c])
            if l == 0:
                raise JpegStreamError(1, self.name)
            bits.skip(l)
            st["symbols"] += 1
            st["max_code_length"] = max(st["max_code_length"], l)
            return int(tab[1][c])

        def wrap16(v):
            return ((v + 0x8000) & 0xFFFF) - 0x8000

        pred = [0, 0, 0]
        eobrun = 0
        n_mcu = len(order) // per_mcu
        for mcu in range(n_mcu):
            if sc.restart_interval and mcu and mcu % sc.restart_interval == 0:
                bits.restart()
                st["restarts"] += 1
                pred = [0, 0, 0]
                eobrun = 0
            for r in range(per_mcu):
                blk = coef[int(order[mcu * per_mcu + r])]
                j = 0 if per_mcu == 1 else (0 if r < luma else 1 + r - luma)      # which of the scan's components
                if ss == 0 and ah == 0:                          # DC first
                    t = symbol(looks[j])
                    if t > 15:
                        raise JpegStreamError(5, self.name)
                    st["max_dc_category"] = max(st["max_dc_category"], t)
                    if t:
                        pred[j] += bits.receive_extend(t)
                    blk[0] = wrap16(pred[j] << al)
                elif ss == 0:                                    # DC refinement
                    if bits.take(1):
                        blk[0] = wrap16(int(blk[0]) | p1)
                elif ah == 0:                                    # AC first
                    if eobrun > 0:
                        eobrun -= 1
                        continue
                    k = ss
                    while k <= se:
                        rs = symbol(looks[0])
                        run, size = rs >> 4, rs & 15
                        if size:
                            k += run
                            if k > se:
                                raise JpegStreamError(2, self.name)
                            blk[zz[k]] = wrap16(bits.receive_extend(size) << al)
                            k += 1
                        elif run == 15:
                            st["zrl"] += 1
                            k += 16
                            if k > se + 1:
                                raise JpegStreamError(2, self.name)
                        else:
                            eobrun = (1 << run) + (bits.take(run) if run else 0)
                            st["eobrun_max"] = max(st["eobrun_max"], eobrun)
                            eobrun -= 1
                            break
                else:                                            # AC refinement
                    k = ss
                    if eobrun == 0:
                        while k <= se:
                            rs = symbol(looks[0])
                            run, size = rs >> 4, rs & 15
                            value = 0
                            if size:
                                if size != 1:
                                    raise JpegStreamError(1, self.name)
                                value = p1 if bits.take(1) else m1
                            elif run != 15:
                                eobrun = (1 << run) + (bits.take(run) if run else 0)
                                st["eobrun_refine_max"] = max(st["eobrun_refine_max"], eobrun)
                                break
                            else:
                                st["zrl_refine"] += 1
                            while k <= se:                       # over the coefficients that are known, and `run` that are not
                                v = int(blk[zz[k]])
                                if v:
                                    st["correction_bits"] += 1
                                    if bits.take(1) and not v & p1:
                                        blk[zz[k]] = wrap16(v + (p1 if v > 0 else m1))
                                else:
                                    run -= 1
                                    if run < 0:
                                        break
                                k += 1
                            if value:
                                if k > se:
                                    raise JpegStreamError(2, self.name)
                                blk[zz[k]] = wrap16(value)
                            k += 1
                    if eobrun > 0:
                        while k <= se:
                            v = int(blk[zz[k]])
                            if v:
                                st["correction_bits"] += 1
                                if bits.take(1) and not v & p1:
                                    blk[zz[k]] = wrap16(v + (p1 if v > 0 else m1))
                            k += 1
                        eobrun -= 1

    # ---- the parallel entropy stage in Python (csrc/jpeg_sync.h) ---------------------------------------------------------
    def _sync_context(self):
        self._require()
        if self.progressive:
            raise ValueError("JPEG image %s is progressive: the parallel entropy stage decodes baseline scans" % self.name)
        _, huff = self._tables
        hs, vs = self.luma_sampling
        nc = len(self.components)
        tabs = {}
        for key, (cnt, sy) in huff.items():                  # 16-bit prefix -> length (0: no code) and symbol, as bytes
            ln, sv = bytearray(1 << 16), bytearray(1 << 16)
            code, k = 0, 0
            for l in range(1, 17):
                for _ in range(int(cnt[l - 1])):
                    if code >= 1 << l:
                        raise ValueError("JPEG %s: Huffman code lengths that form no prefix code" % self.name)
                    lo, span = code << (16 - l), 1 << (16 - l)
                    ln[lo:lo + span] = bytes([l]) * span
                    sv[lo:lo + span] = bytes([int(sy[k])]) * span
                    code += 1
                    k += 1
                code <<= 1
            tabs[key] = (bytes(ln), bytes(sv))
        sel = list(self.scan_tables) + [self.scan_tables[0]] * (3 - nc)
        mw, mh = -(-self.W // (8 * hs)), -(-self.H // (8 * vs))
        bpm = hs * vs + (2 if nc == 3 else 0)
        return dict(p=self.entropy_bytes(), luma=hs * vs, bpm=bpm, ri=self.restart_interval, n_blocks=mw * mh * bpm,
                    dc=[tabs[(0, td)] for td, ta in sel], ac=[tabs[(1, ta)] for td, ta in sel])

    @staticmethod
    def _sync_decode(cx, sub_end, max_passes, e_byte, e_brk, e_m, store=None):
        """``jpeg_sync_decode`` of csrc/jpeg_sync.h, statement by statement.  store: None, or (coef int16 [n_blocks, 64],
        first block, (p0, p1, p2)) for the write pass.  Returns (byte, brk, m, blocks, d0, d1, d2, markers, marker delta,
        blocks before the first marker, blocks before the first violation or -1)."""
        p, luma, bpm, ri, dct, act = cx["p"], cx["luma"], cx["bpm"], cx["ri"], cx["dc"], cx["ac"]
        end = len(p)
        n_blocks = cx["n_blocks"]
        pos = min(max(e_byte, 0), end)
        acc, n, stall = 0, 0, 0
        units = []                                           # raw index of every byte unit taken since acc was last empty
        r, k, m = (e_brk >> 8) & 255, (e_brk >> 16) & 255, e_m
        if r >= bpm:
            r = 0
        if k > 63:
            k = 0
        blocks, nrst, rst_delta, rst_blocks, viol = 0, 0, 0, 0, -1
        d = [0, 0, 0]
        if store is not None:
            coef, first_block, pr = store
            pr = list(pr)
        first = True
        passes = 0
        while True:
            if not first:
                if passes >= max_passes:
                    if viol < 0:
                        viol = blocks
                    break
                if store is not None and first_block + blocks >= n_blocks:
                    break
            while n < 32 and not stall:                      # jpeg_sync_refill
                if pos >= end:
                    stall = 1
                elif p[pos] != 0xFF:
                    acc = ((acc << 8) | p[pos]) & 0xFFFFFFFFFFFFFFFF
                    units.append(pos)
                    pos += 1
                    n += 8
                elif pos + 1 >= end:
                    stall = 1
                elif p[pos + 1] != 0:
                    stall = 2
                else:
                    acc = ((acc << 8) | 0xFF) & 0xFFFFFFFFFFFFFFFF
                    units.append(pos)
                    pos += 2
                    n += 8
            if first:                                        # the bits of the entry's byte unit that are used already
                first = False
                bit = e_brk & 7
                if bit and n >= 8:
                    n -= bit
                continue
            nb = (n + 7) >> 3
            if (units[len(units) - nb] if nb else pos) >= sub_end:
                break
            passes += 1
            at_marker = False
            if ri > 0 and r == 0 and k == 0 and m >= ri:
                if n >= 8:
                    if viol < 0:
                        viol = blocks
                    m = 0
                elif stall == 1:
                    break
                else:
                    at_marker = True
            if not at_marker:
                w = ((acc >> (n - 32)) if n >= 32 else (acc << (32 - n))) & 0xFFFFFFFF
                comp = 0 if r < luma else 1 + (r - luma)
                tab = dct[comp] if k == 0 else act[comp]
                length = tab[0][w >> 16]
                sym = tab[1][w >> 16] if length else -1
                if sym < 0 and not (stall and n < 16):
                    if viol < 0:
                        viol = blocks
                    n -= 1
                    continue
                size = sym if k == 0 else sym & 15
                if k == 0 and sym > 15:
                    if viol < 0:
                        viol = blocks
                    size = 0
                if sym < 0 or length + size > n:
                    if stall != 2:
                        break
                    if viol < 0:
                        viol = blocks
                    at_marker = True
                else:
                    val = 0
                    if size:
                        v = ((w << length) & 0xFFFFFFFF) >> (32 - size)
                        val = v if v >= 1 << (size - 1) else v - (1 << size) + 1
                    n -= length + size
                    if k == 0:
                        d[comp] += val
                        if store is not None:
                            pr[comp] += val
                            if first_block + blocks < n_blocks:
                                coef[first_block + blocks, 0] = np.int64(pr[comp]).astype(np.int16)
                        k = 1
                    else:
                        run = sym >> 4
                        if size == 0:
                            if run == 15:
                                k += 16
                                if k > 64:
                                    if viol < 0:
                                        viol = blocks
                                    k = 64
                            else:
                                k = 64
                        else:
                            k += run
                            if k > 63:
                                if viol < 0:
                                    viol = blocks
                                k = 64
                            else:
                                if store is not None and first_block + blocks < n_blocks:
                                    coef[first_block + blocks, ZIGZAG[k]] = val
                                k += 1
                    if k >= 64:
                        k = 0
                        blocks += 1
                        r += 1
                        if r >= bpm:
                            r = 0
                            if ri > 0:
                                m += 1
                    continue
            if stall != 2:
                break
            x = p[pos + 1]
            if x == 0xFF:
                pos += 1
            elif x & 0xF8 == 0xD0:
                dl = (x - nrst) & 7
                if nrst == 0:
                    rst_delta, rst_blocks = dl, blocks
                elif dl != rst_delta and viol < 0:
                    viol = blocks
                nrst += 1
                pos += 2
                r = k = m = 0
                d = [0, 0, 0]
                if store is not None:
                    pr = [0, 0, 0]
            else:
                if viol < 0:
                    viol = blocks
                break
            n, stall = 0, 0
            del units[:]
        nb = (n + 7) >> 3
        byte = units[len(units) - nb] if nb else pos
        return (byte, ((8 - (n & 7)) & 7) | (r << 8) | (k << 16), m, blocks, d[0] & 0xFFFFFFFF, d[1] & 0xFFFFFFFF,
                d[2] & 0xFFFFFFFF, nrst, rst_delta, rst_blocks, viol)

    def parallel_plan(self, subseq_bytes, max_rounds, coefficients=False):
        """What the parallel entropy stage (``io_jpeg_decode_par_u8``) does with this file, by the rule of csrc/jpeg_sync.h
        in Python: dict(rounds, subsequences, live, decodes, fallback, blocks).  ``rounds | fallback`` is the info word of
        the image: fallback is 0, 1 << 16 (no convergence within max_rounds) or 1 << 17 (converged, not clean); the
        sequential stage decodes an image with a fallback.  live: subsequences up to the one that completes the last
        block (0 with a fallback); decodes: subsequence decodes of all rounds; blocks: blocks per live subsequence.
        With ``coefficients`` a clean image also gets "coefficients", the int16 [n_blocks, 64] of the write pass."""
        if subseq_bytes % 8 or not 16 <= subseq_bytes <= 4096 or not 1 <= max_rounds <= 65535:
            raise ValueError("parallel_plan: subseq_bytes %d (a multiple of 8 in 16..4096), max_rounds %d (1..65535)"
                             % (subseq_bytes, max_rounds))
        cx = self._sync_context()
        p = cx["p"]
        nbytes, n_blocks = len(p), cx["n_blocks"]
        nsub = max(1, -(-nbytes // subseq_bytes))
        ends = [min((i + 1) * subseq_bytes, nbytes) for i in range(nsub)]
        entry = [(0, 0, 0)]
        for i in range(1, nsub):                             # jpeg_sync_guess
            g = min(i * subseq_bytes, nbytes)
            if 1 <= g < nbytes and p[g - 1] == 0xFF and (p[g] == 0 or p[g] & 0xF8 == 0xD0):
                g += 1
            entry.append((g, 0, 0))
        changed = [True] * nsub
        exits = [None] * nsub
        rounds, decodes, converged = 0, 0, False
        passes = 8 * subseq_bytes + 32
        while rounds < max_rounds and not converged:
            for i in range(nsub):
                if changed[i]:
                    exits[i] = self._sync_decode(cx, ends[i], passes, *entry[i])
                    decodes += 1
            rounds += 1
            converged = True
            changed[0] = False
            for i in range(1, nsub):
                changed[i] = exits[i - 1][:3] != entry[i]
                entry[i] = exits[i - 1][:3]
                if changed[i]:
                    converged = False
        out = dict(rounds=rounds, subsequences=nsub, live=0, decodes=decodes, fallback=0, blocks=[])
        if not converged:
            out["fallback"] = 1 << 16
            return out
        first, markers, clean, full = 0, 0, True, False      # jpeg_sync_finish
        pred = [0, 0, 0]
        starts = []
        for i in range(nsub):
            byte, brk, m, blocks, d0, d1, d2, nrst, delta, rst_blocks, viol = exits[i]
            starts.append((first, tuple(v & 0xFFFF for v in pred)))
            if viol >= 0 and first + viol < n_blocks:
                clean = False
            if nrst > 0:
                if first + rst_blocks < n_blocks and delta != markers & 7:
                    clean = False
                markers += nrst
                pred = [0, 0, 0]
            pred = [(a + (b & 0xFFFF)) & 0xFFFFFFFF for a, b in zip(pred, (d0, d1, d2))]
            first += blocks
            out["blocks"].append(blocks)
            if first >= n_blocks:
                full = True
                break
        if not (clean and full):
            out["fallback"] = 1 << 17
            out["blocks"] = []
            return out
        out["live"] = len(starts)
        if coefficients:
            coef = np.zeros((n_blocks, 64), np.int16)
            for i, (fb, pr) in enumerate(starts):
                self._sync_decode(cx, ends[i], passes, *entry[i], store=(coef, fb, pr))
            out["coefficients"] = coef
        return out

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


def _lookup(counts, symbols, name):
    """16-bit prefix -> (code length or 0, symbol) of one Huffman table given as the bytes of its DHT entry"""
    ln = np.zeros(1 << 16, np.uint8)
    sv = np.zeros(1 << 16, np.uint8)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            if code >= 1 << l:
                raise ValueError("JPEG %s: Huffman code lengths that form no prefix code" % name)
            lo = code << (16 - l)
            ln[lo:lo + (1 << (16 - l))] = l
            sv[lo:lo + (1 << (16 - l))] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return ln, sv


class _Bits(object):
    """the bits of one entropy-coded segment: FF fill bytes dropped, FF 00 unstuffed, split at the restart markers; inside
    an interval the reader stops at any other marker.  Raises the JpegStreamError the kernel's status word stands for."""

    def __init__(self, raw, name):
        self.name = name
        raw = _FILL.sub(b"", raw)
        segs, self.marks, at = [], [], 0
        for mt in _RST.finditer(raw):
            segs.append(raw[at:mt.start()])
            self.marks.append(raw[mt.end() - 1] - 0xD0)
            at = mt.end()
        segs.append(raw[at:])
        self.clean, self.cut = [], []
        for sg in segs:
            mt = _MARKER.search(sg)
            self.cut.append(mt is not None)
            if mt:
                sg = sg[:mt.start()]
            self.clean.append(sg.replace(b"\xff\x00", b"\xff"))
        self.seg = -1
        self._enter(0)

    def _enter(self, k):
        self.seg, self.buf, self.bits, self.pos = k, self.clean[k] + b"\0" * 8, 8 * len(self.clean[k]), 0

    def peek16(self):
        p = self.pos
        return (int.from_bytes(self.buf[p >> 3:(p >> 3) + 4], "big") >> (16 - (p & 7))) & 0xFFFF

    def skip(self, k):
        self.pos += k
        if self.pos > self.bits:
            raise JpegStreamError(4, self.name)

    def take(self, s):
        """the next s bits (1 <= s <= 15) as an unsigned number"""
        v = self.peek16() >> (16 - s)
        self.skip(s)
        return v

    def receive_extend(self, s):
        v = self.take(s)
        return v if v >= 1 << (s - 1) else v - (1 << s) + 1

    def restart(self):
        k = self.seg
        if self.bits - self.pos >= 8 or self.cut[k] or k >= len(self.marks) or self.marks[k] != k % 8:
            raise JpegStreamError(3, self.name)
        self._enter(k + 1)


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


def descriptors_progressive(images, out_offs):
    """dict(pool, tables, huff, desc, image, scan) for a list of accepted progressive ``JpegImage`` and the byte offset of
    each decoded image: what ``io_jpeg_decode_prog_u8`` reads.  pool: the entropy-coded bytes of all scans; tables: uint8
    [n_sets * 1600], the quantisation tables (identical sets stored once); huff: uint8 [n_huff * 272], the raw Huffman
    tables (identical tables stored once); desc / image / scan: the JpegDesc, JpegProgImage and JpegProgScan arrays."""
    n_scans = sum(len(im.scans) for im in images)
    desc = (_lib.JpegDesc * len(images))()
    recs = (_lib.JpegProgImage * len(images))()
    scans = (_lib.JpegProgScan * max(n_scans, 1))()
    sets, blobs, tabs, chunks, cursor, g = {}, [], {}, [], 0, 0
    for k, (im, o) in enumerate(zip(images, out_offs)):
        im._require()
        if not im.progressive:
            raise ValueError("jpeg.descriptors_progressive: %s is a baseline file" % im.name)
        blob = im.tables_blob()
        if blob not in sets:
            sets[blob] = len(blobs)
            blobs.append(blob)
        d = desc[k]
        d.out_off, d.H, d.W, d.n_comp = int(o), im.H, im.W, len(im.components)
        d.hs, d.vs = im.luma_sampling
        d.table_set = sets[blob]
        for c, (cid, h, v, tq) in enumerate(im.components):
            d.quant[c] = tq
        levels = im.scan_levels()
        recs[k].first_scan, recs[k].n_scans, recs[k].n_levels = g, len(im.scans), max(levels) + 1
        for n, (sc, lv) in enumerate(zip(im.scans, levels)):
            s = scans[g]
            ent = im.scan_bytes(n)
            s.data_off, s.data_bytes, s.image, s.restart_interval, s.level = cursor, len(ent), k, sc.restart_interval, lv
            s.n_comp, s.ss, s.se, s.ah, s.al = len(sc.comps), sc.ss, sc.se, sc.ah, sc.al
            for j, (c, t) in enumerate(zip(sc.comps, sc.tables)):
                s.comp[j] = c
                if t is not None:
                    s.table[j] = tabs.setdefault(t, len(tabs))
            chunks.append(ent)
            cursor += len(ent)
            g += 1
    pool = np.frombuffer(b"".join(chunks), np.uint8) if cursor else np.zeros(0, np.uint8)
    huff = np.zeros((max(len(tabs), 1), 272), np.uint8)
    for (cnt, sy), t in tabs.items():
        huff[t, :16] = np.frombuffer(cnt, np.uint8)
        huff[t, 16:16 + len(sy)] = np.frombuffer(sy, np.uint8)
    return dict(pool=pool, tables=np.frombuffer(b"".join(blobs), np.uint8), huff=huff.reshape(-1), desc=desc, image=recs,
                scan=scans, n_scans=n_scans)


def workspace_bytes_progressive(p):
    """bytes of workspace ``io_jpeg_decode_prog_u8`` needs for the tables of ``descriptors_progressive``"""
    b = int(_lib.lib().io_jpeg_prog_workspace_bytes(C.cast(p["desc"], C.c_void_p), len(p["desc"]), p["huff"].size // 272,
                                                    p["n_scans"]))
    if b == 0:
        raise RuntimeError("instaorder_hip io_jpeg_prog_workspace_bytes refused the descriptors: %s" % _lib.last_error())
    return b


def progressive_blobs(p):
    """the uint8 arrays of ``p`` that travel to the device, in the order (tables, huff, desc, image, scan, pool)"""
    return [p["tables"], p["huff"], np.frombuffer(p["desc"], dtype=np.uint8), np.frombuffer(p["image"], dtype=np.uint8),
            np.frombuffer(p["scan"], dtype=np.uint8), p["pool"]]


# ---- which entropy stage the device decoder runs --------------------------------------------------------------------------
_ENTROPY = dict(mode="sequential", subseq_bytes=256, max_rounds=64)


def set_entropy(mode, subseq_bytes=256, max_rounds=64):
    """The entropy stage of ``decode`` and of ``datasets.PairRenderer`` (so of the ``*Batches`` classes, the inference
    drivers and ``evaluate``): "sequential", one lane per image (``io_jpeg_decode_u8``), or "parallel", the lanes of a
    workgroup on the subsequences of one image (``io_jpeg_decode_par_u8``, csrc/jpeg_sync.h).  Pixels and status words do
    not depend on it.  Module-wide; the default is "sequential", the environment variable IO_JPEG_ENTROPY=parallel selects
    the other at import.  Any other non-empty value of that variable raises this function's ValueError when
    ``instaorder_amd.jpeg`` is imported: a misspelt setting stops the program instead of running the other stage."""
    if mode not in ("sequential", "parallel"):
        raise ValueError("jpeg.set_entropy: mode %r ('sequential' or 'parallel')" % (mode,))
    if subseq_bytes % 8 or not 16 <= subseq_bytes <= 4096 or not 1 <= max_rounds <= 65535:
        raise ValueError("jpeg.set_entropy: subseq_bytes %d (a multiple of 8 in 16..4096), max_rounds %d (1..65535)"
                         % (subseq_bytes, max_rounds))
    _ENTROPY.update(mode=mode, subseq_bytes=int(subseq_bytes), max_rounds=int(max_rounds))


def get_entropy(entropy=None):
    """dict(mode, subseq_bytes, max_rounds): the module setting, with ``entropy`` ("sequential" / "parallel") in place of
    its mode; such a dict is returned as it is"""
    if isinstance(entropy, dict):
        return dict(entropy)
    e = dict(_ENTROPY)
    if entropy is not None:
        if entropy not in ("sequential", "parallel"):
            raise ValueError("jpeg: entropy %r ('sequential' or 'parallel')" % (entropy,))
        e["mode"] = entropy
    return e


if os.environ.get("IO_JPEG_ENTROPY", ""):
    set_entropy(os.environ["IO_JPEG_ENTROPY"])


# ---- who decodes a progressive file -----------------------------------------------------------------------------------------
_PROGRESSIVE = dict(mode="host", concurrent=1)


def set_progressive(mode, concurrent=1):
    """Who decodes a progressive (SOF2) file: "host" -- ``JpegImage.supported`` is False with "progressive" in its reason
    and ``loader`` hands the file to its fallback, the default -- or "device": ``JpegImage`` accepts the progressive files
    of DESIGN.md "Progressive JPEG" and ``io_jpeg_decode_prog_u8`` decodes them.  ``concurrent`` (1 or 0): the scans of one
    level side by side on the waves of a block, or all scans in file order on one lane; pixels and status words do not
    depend on it.  Module-wide; applies to ``JpegImage`` objects made afterwards.  The environment variable
    IO_JPEG_PROGRESSIVE=device selects the device at import; any other non-empty value of it raises this function's
    ValueError when ``instaorder_amd.jpeg`` is imported."""
    if mode not in ("host", "device"):
        raise ValueError("jpeg.set_progressive: mode %r ('host' or 'device')" % (mode,))
    if concurrent not in (0, 1):
        raise ValueError("jpeg.set_progressive: concurrent %r (0 or 1)" % (concurrent,))
    _PROGRESSIVE.update(mode=mode, concurrent=int(concurrent))


def get_progressive():
    return _PROGRESSIVE["mode"]


if os.environ.get("IO_JPEG_PROGRESSIVE", ""):
    set_progressive(os.environ["IO_JPEG_PROGRESSIVE"])


def workspace_bytes(desc, entropy=None):
    e = get_entropy(entropy)
    if e["mode"] == "parallel":
        fn = "io_jpeg_par_workspace_bytes"
        b = int(_lib.lib().io_jpeg_par_workspace_bytes(C.cast(desc, C.c_void_p), len(desc), e["subseq_bytes"]))
    else:
        fn = "io_jpeg_workspace_bytes"
        b = int(_lib.lib().io_jpeg_workspace_bytes(C.cast(desc, C.c_void_p), len(desc)))
    if b == 0:
        raise RuntimeError("instaorder_hip %s refused the descriptors: %s" % (fn, _lib.last_error()))
    return b


def group(images, entropy=None):
    """``arena.Group`` of the baseline files ``images``: blobs (pool, tables, JpegDesc array), one ``io_jpeg_decode_u8`` or
    ``io_jpeg_decode_par_u8`` call as ``entropy`` (a mode, a ``get_entropy`` dict, None: the ``set_entropy`` setting) says
    -- the same setting sizes the workspace -- and a status word per image; ``info``: the address of n int32 or None."""
    if not images:
        return arena.Group()
    e = get_entropy(entropy)
    pool, tables, desc = descriptors(images, [0] * len(images))

    def launch(addrs, out, out_bytes, ws, ws_bytes, status, stream, info=None):
        head = (C.c_void_p(addrs[0]), C.c_size_t(pool.size), C.c_void_p(addrs[1]), tables.ctypes.data_as(C.c_void_p),
                C.c_size_t(tables.size), C.c_void_p(addrs[2]), C.cast(desc, C.c_void_p), len(desc), C.c_void_p(out),
                C.c_size_t(out_bytes), C.c_void_p(ws), C.c_size_t(ws_bytes), C.c_void_p(status))
        if e["mode"] == "parallel":
            fn = "io_jpeg_decode_par_u8"
            rc = _lib.lib().io_jpeg_decode_par_u8(*(head + (e["subseq_bytes"], e["max_rounds"],
                                                            C.c_void_p(info) if info else None, C.c_void_p(stream))))
        else:
            fn = "io_jpeg_decode_u8"
            rc = _lib.lib().io_jpeg_decode_u8(*(head + (C.c_void_p(stream),)))
        _lib.check(rc, fn)

    return arena.Group([pool, tables, arena.as_bytes(desc)], ("images", "images", "descriptors"), desc, launch,
                       lambda: workspace_bytes(desc, e), images, raise_for_status)


def group_progressive(images, concurrent=None):
    """``arena.Group`` of the accepted progressive files ``images``: the blobs of ``progressive_blobs``, one
    ``io_jpeg_decode_prog_u8`` call (``concurrent``: 1 or 0 instead of the ``set_progressive`` value) with a workspace, and
    a status word per image"""
    if not images:
        return arena.Group()
    concurrent = _PROGRESSIVE["concurrent"] if concurrent is None else int(concurrent)
    p = descriptors_progressive(images, [0] * len(images))

    def launch(addrs, out, out_bytes, ws, ws_bytes, status, stream, info=None):
        tables_dev, huff_dev, desc_dev, image_dev, scan_dev, pool_dev = addrs
        rc = _lib.lib().io_jpeg_decode_prog_u8(
            C.c_void_p(pool_dev), C.c_size_t(p["pool"].size), C.c_void_p(tables_dev), p["tables"].ctypes.data_as(C.c_void_p),
            C.c_size_t(p["tables"].size), C.c_void_p(huff_dev), p["huff"].ctypes.data_as(C.c_void_p), p["huff"].size // 272,
            C.c_void_p(desc_dev), C.cast(p["desc"], C.c_void_p), C.c_void_p(image_dev), C.cast(p["image"], C.c_void_p),
            len(p["desc"]), C.c_void_p(scan_dev), C.cast(p["scan"], C.c_void_p), p["n_scans"], C.c_void_p(out),
            C.c_size_t(out_bytes), C.c_void_p(ws), C.c_size_t(ws_bytes), C.c_void_p(status), concurrent, C.c_void_p(stream))
        _lib.check(rc, "io_jpeg_decode_prog_u8")

    return arena.Group(progressive_blobs(p), ("images", "images", "descriptors", "descriptors", "descriptors", "images"),
                       p["desc"], launch, lambda: workspace_bytes_progressive(p), images, raise_for_status)


def raise_for_status(status, images):
    """RuntimeError naming the images whose status word is not zero"""
    bad = [(im.name, int(s)) for im, s in zip(images, status) if int(s) != 0]
    if bad:
        raise RuntimeError("JPEG decode failed: " + "; ".join("%s: %s (status %d)" % (nm, STATUS.get(s, "?"), s)
                                                               for nm, s in bad))


def decode(images, device, out=None, entropy=None, info=False, concurrent=None):
    """list of supported ``JpegImage`` -> list of uint8 [H, W, 3] device tensors through one ``io_jpeg_decode_u8`` call on
    the current stream (views of ``out``, a contiguous uint8 device tensor of at least the summed sizes, when given).
    Waits for the status words and raises RuntimeError naming the images that did not decode.  ``entropy``: "sequential"
    or "parallel" instead of the ``set_entropy`` mode.  With ``info`` the result is (tensors, int32 array): the info word
    of every image (``JpegImage.parallel_plan``; zeros from the sequential stage).  Baseline and accepted progressive
    images may be mixed: the baseline ones go through that call, the progressive ones through one ``io_jpeg_decode_prog_u8``
    call (``concurrent``: 1 or 0 instead of the ``set_progressive`` value) into the same output and one status vector."""
    import torch
    _lib.require_gpu()
    device = torch.device(device)
    images = list(images)
    setting = get_entropy(entropy)
    if not images:
        return ([], np.zeros(0, np.int32)) if info else []
    for im in images:
        if not is_jpeg(im):
            raise TypeError("jpeg.decode takes JpegImage objects (got %s)" % type(im).__name__)
        im._require()
    sizes = [im.H * im.W * 3 for im in images]
    lay = arena.Layout()
    offs = [lay.add(s) for s in sizes]
    total = offs[-1] + sizes[-1]
    if out is None:
        out = torch.empty(total, dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() < total:
        raise ValueError("jpeg.decode: out must be a contiguous uint8 device tensor of at least %d bytes" % total)
    out = out.view(-1)
    base_idx = [k for k, im in enumerate(images) if not im.progressive]
    prog_idx = [k for k, im in enumerate(images) if im.progressive]
    groups = [group([images[k] for k in base_idx], setting), group_progressive([images[k] for k in prog_idx], concurrent)]
    groups[0].set_outs(offs[k] for k in base_idx)
    groups[1].set_outs(offs[k] for k in prog_idx)
    # one status vector: the words of the baseline images, then those of the progressive ones
    status = torch.empty(len(images), dtype=torch.int32, device=out.device)
    words = torch.zeros(len(images), dtype=torch.int32, device=out.device)
    arena.decode_into(groups, out, status, words if info else None)
    order = base_idx + prog_idx
    if prog_idx and base_idx:
        back = torch.from_numpy(np.argsort(order))
        status, words = status.cpu()[back], words.cpu()[back]
    raise_for_status(status.cpu().numpy(), images)
    res = [out[o:o + s].view(im.H, im.W, 3) for o, s, im in zip(offs, sizes, images)]
    return (res, words.cpu().numpy()) if info else res


def _pil_rgb(path):
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("jpeg.loader: %s is not a JPEG file the device decoder takes and the default fallback needs "
                           "Pillow, which is not installed; pass fallback=" % path)
    return np.array(Image.open(path).convert("RGB"))


def loader(image_root, fallback=None, progressive=None):
    """``load_image(image_fn)`` for the dataset classes: a ``JpegImage`` for a file the device decodes, otherwise
    ``fallback(path)`` -- by default the reference's own ``np.array(Image.open(path).convert('RGB'))``.  ``progressive``:
    True / False, whether progressive files go to the device; None: as ``set_progressive`` says when a file is loaded."""
    fallback = _pil_rgb if fallback is None else fallback

    def load_image(image_fn):
        path = os.path.join(image_root, image_fn)
        with open(path, "rb") as f:
            data = f.read()
        if data[:2] == b"\xff\xd8":
            try:
                im = JpegImage(data, name=str(image_fn), progressive=progressive)
            except ValueError:
                im = None
            if im is not None and im.supported:
                return im
        return fallback(path)

    return load_image
