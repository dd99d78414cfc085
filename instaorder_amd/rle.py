"""Run-length-encoded instance masks (COCO RLE) for the device input pipeline.

Of the reference's datasets KINS, and the crowd regions of COCO (InstaOrder, COCOA), store their masks as COCO run-length
codes; every other COCO instance is a list of polygons (``poly.PolyMasks`` carries those, and codes mixed in with them).
The reference decodes both to dense [n, H, W] arrays on the host only because a cv2 pipeline needs pixels.  Here the
codes travel to the GPU as they are -- a few hundred uint32 per mask instead of H * W bytes -- and ``io_rle_decode_u8``
(csrc/rle.hip) decodes them there, in front of the render kernel (``datasets.PairRenderer``) and of the mask rules
(``mask_rules``).

The format: a mask of H x W is a list of non-negative run lengths over its pixels in COLUMN-major order (q = x * H + y).
Runs alternate 0, 1, 0, ... and start with a run of zeros, so a mask whose first pixel is set starts with the count 0;
zero-length runs may appear anywhere; the counts sum to H * W.  With ``ends = cumsum(counts)`` pixel q lies in run
``r = #{k : ends[k] <= q}`` and has the value ``r & 1`` -- repeated entries of ``ends`` need no special case.

Opt-in: dense masks keep their code path.  ``RLEReader`` turns any ``data_reader`` into one that hands out ``RLEMasks``.
"""
import ctypes as C

import numpy as np

from . import _lib, arena


def _counts_from_string(s):
    """The compressed string form of COCO RLE -> counts: 5-bit groups, low group first, as ASCII characters offset by 48,
    bit 0x20 = another group follows, bit 0x10 of the last group = sign; every count from the fourth on (index >= 3) is
    stored as the difference from the count two places before it."""
    if isinstance(s, str):
        s = s.encode("ascii")
    counts, p, n = [], 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ValueError("RLE string ends inside a count")
            c = s[p] - 48
            if not 0 <= c < 64:
                raise ValueError("RLE string: character %r outside the code alphabet" % chr(s[p]))
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


class EncodedMasks(object):
    """What the consumers test for: the n instance masks of one image in a form that stays encoded up to the device
    (``RLEMasks``, ``poly.PolyMasks``).  A subclass offers ``shape``, ``__len__``, ``__getitem__``, ``values``,
    ``with_values``, ``to_dense()`` (host) and ``to_device(device, out=None)`` (uint8 [n, H, W] device tensor)."""


def is_encoded(masks):
    return isinstance(masks, EncodedMasks)


class RLEMasks(EncodedMasks):
    """The n instance masks of one image as run-length codes: ``counts`` is a list of n sequences of run lengths, ``values``
    the byte each mask carries where it is set (1, or a category id).  Stands in for a uint8 [n, H, W] array wherever the
    renderer, the dataset classes, ``mask_rules`` and the inference drivers take one."""

    def __init__(self, counts, H, W, values=None):
        H, W = int(H), int(W)
        if H <= 0 or W <= 0 or H * W >= 1 << 31:
            raise ValueError("RLEMasks: size %d x %d (need H, W > 0 and H * W < 2^31)" % (H, W))
        cs = []
        for i, c in enumerate(counts):
            a = np.asarray(c)
            if a.ndim != 1 or a.size == 0:
                raise ValueError("RLEMasks: mask %d: counts must be a non-empty 1-D sequence" % i)
            if a.dtype.kind not in ("u", "i"):
                raise ValueError("RLEMasks: mask %d: counts must be integers (got %s)" % (i, a.dtype))
            a64 = a.astype(np.int64)
            if (a64 < 0).any():
                raise ValueError("RLEMasks: mask %d has a negative run length" % i)
            if int(a64.sum()) != H * W:
                raise ValueError("RLEMasks: mask %d: run lengths sum to %d, the image has %d x %d = %d pixels"
                                 % (i, int(a64.sum()), H, W, H * W))
            cs.append(a64.astype(np.uint32))
        self._counts = cs
        self.H, self.W = H, W
        n = len(cs)
        if values is None:
            v = np.ones(n, np.int64)
        else:
            v = np.asarray(values)
            if v.dtype.kind not in ("u", "i", "b"):
                raise ValueError("RLEMasks: values must be integers (got %s)" % v.dtype)
            v = np.broadcast_to(v.astype(np.int64), (n,)).copy()
            if n and (v.min() < 0 or v.max() > 255):
                raise ValueError("RLEMasks: values must lie in 0..255")
        self.values = v
        self._ends = None

    # ---- the part of the array interface the consumers use ----------------------------------------------------------
    @property
    def shape(self):
        return (len(self._counts), self.H, self.W)

    def __len__(self):
        return len(self._counts)

    @property
    def counts(self):
        return self._counts

    def __getitem__(self, idx):
        """Instances by index: an int gives the one-mask RLEMasks (shape (1, H, W)), a list / array / slice the subset."""
        n = len(self)
        if isinstance(idx, (int, np.integer)):
            sel = [range(n)[idx]]
        elif isinstance(idx, slice):
            sel = list(range(n))[idx]
        else:
            a = np.asarray(idx)
            if a.dtype.kind == "b":
                if a.shape != (n,):
                    raise IndexError("boolean index of shape %s for %d masks" % (a.shape, n))
                sel = list(np.nonzero(a)[0])
            elif a.ndim == 1 and (a.dtype.kind in ("u", "i") or a.size == 0):
                sel = [range(n)[int(i)] for i in a]
            else:
                raise IndexError("RLEMasks are indexed by instance: an int, a slice or a 1-D list of ints")
        out = RLEMasks.__new__(RLEMasks)
        out._counts = [self._counts[i] for i in sel]
        out.H, out.W = self.H, self.W
        out.values = self.values[[int(i) for i in sel]] if sel else np.zeros(0, np.int64)
        out._ends = None
        return out

    def with_values(self, category):
        """The same masks carrying ``category`` (a scalar or one id per mask) where they are set -- the reference's
        ``modal * category[:, None, None]``.  Shares the codes."""
        out = RLEMasks.__new__(RLEMasks)
        out._counts = self._counts
        out.H, out.W = self.H, self.W
        v = np.asarray(category)
        if v.dtype.kind not in ("u", "i", "b"):
            raise ValueError("RLEMasks.with_values: integer ids expected (got %s)" % v.dtype)
        v = np.broadcast_to(v.astype(np.int64), (len(self),)).copy()
        if len(self) and (v.min() < 0 or v.max() > 255):
            raise ValueError("RLEMasks.with_values: values must lie in 0..255")
        out.values = v
        out._ends = self._ends
        return out

    def ends(self):
        """(ends, offsets): the inclusive prefix sums of all masks concatenated (uint32) and offsets int64 [n + 1], mask i
        owning ends[offsets[i]:offsets[i + 1]] -- the run table ``io_rle_decode_u8`` reads."""
        if self._ends is None:
            offsets = np.zeros(len(self) + 1, np.int64)
            if len(self):
                offsets[1:] = np.cumsum([c.size for c in self._counts])
                ends = np.concatenate([np.cumsum(c, dtype=np.int64) for c in self._counts]).astype(np.uint32)
            else:
                ends = np.zeros(0, np.uint32)
            self._ends = (ends, offsets)
        return self._ends

    def to_dense(self):
        """uint8 [n, H, W] on the host, by the rule of the module docstring (what host-only code paths use)."""
        n, H, W = self.shape
        out = np.zeros((n, H, W), np.uint8)
        ends, offsets = self.ends()
        q = (np.arange(W, dtype=np.int64)[None, :] * H + np.arange(H, dtype=np.int64)[:, None]).reshape(-1)
        for i in range(n):
            r = np.searchsorted(ends[offsets[i]:offsets[i + 1]], q, side="right")
            out[i] = ((r & 1) * int(self.values[i])).astype(np.uint8).reshape(H, W)
        return out

    def to_device(self, device, out=None):
        return decode(self, device, out=out)

    # ---- constructors -----------------------------------------------------------------------------------------------
    @classmethod
    def from_dense(cls, masks):
        """Encode [n, H, W] masks (bool or integers in 0..255).  A mask that carries one non-zero value v everywhere it is
        set (a category id) keeps it as its value, so ``from_dense(m).to_dense()`` equals m; a mask with two different
        non-zero values has no run-length form and raises ValueError."""
        m = np.asarray(masks)
        if m.ndim != 3:
            raise ValueError("RLEMasks.from_dense: expected [n, H, W], got shape %s" % (m.shape,))
        if m.dtype.kind not in ("b", "u", "i"):
            raise ValueError("RLEMasks.from_dense: bool or integer masks expected (got %s)" % m.dtype)
        n, H, W = m.shape
        if n == 0:
            return cls([], H, W)
        if m.dtype.kind == "b":
            hi = np.ones(n, np.int64)
        else:
            px = m.reshape(n, -1)
            hi = px.max(axis=1).astype(np.int64)
            if int(px.min()) < 0 or int(hi.max()) > 255:
                raise ValueError("RLEMasks.from_dense: values must lie in 0..255")
            if not ((px == 0) | (px == hi.astype(m.dtype)[:, None])).all():
                raise ValueError("RLEMasks.from_dense: a mask with two different non-zero values has no run-length form")
        flat = (m != 0).transpose(0, 2, 1).reshape(n, H * W)                     # column-major pixel order
        padded = np.zeros((n, H * W + 1), bool)                                  # the code starts with a run of zeros
        padded[:, 1:] = flat
        which, pos = np.nonzero(padded[:, 1:] != padded[:, :-1])                 # pixel q starts a new run
        split = np.searchsorted(which, np.arange(n + 1))
        counts = []
        for i in range(n):
            b = np.concatenate([[0], pos[split[i]:split[i + 1]], [H * W]])
            counts.append(np.diff(b).astype(np.uint32))
        return cls(counts, H, W, values=np.where(hi > 0, hi, 1))

    @classmethod
    def from_coco(cls, objs, values=None):
        """From COCO RLE objects ``{'size': [h, w], 'counts': list | str | bytes}`` of one image (all of one size)."""
        objs = list(objs)
        if not objs:
            raise ValueError("RLEMasks.from_coco: no objects (the image size is unknown)")
        H, W = (int(v) for v in objs[0]["size"])
        counts = []
        for i, o in enumerate(objs):
            if tuple(int(v) for v in o["size"]) != (H, W):
                raise ValueError("RLEMasks.from_coco: object %d has size %s, the first %s" % (i, list(o["size"]), [H, W]))
            c = o["counts"]
            counts.append(np.asarray(_counts_from_string(c) if isinstance(c, (str, bytes)) else c, dtype=np.int64))
        return cls(counts, H, W, values=values)


class RLEReader(object):
    """Wraps a ``data_reader`` so that ``get_image_instances`` returns ``RLEMasks`` in place of the dense ``modal``:
    encoded once per image and cached (the same object on every call, so a batch uploads an image it references several
    times once).  Everything else passes through.  The wrapped reader still builds its dense masks on every call; only the
    encoding is cached.  A reader that wants to keep a dataset's masks compressed in memory builds ``RLEMasks`` itself
    (``from_coco`` on the annotation's codes) and needs no wrapper."""

    def __init__(self, reader):
        self._reader = reader
        self._cache = {}

    def __getattr__(self, name):
        if name.startswith("_"):             # not forwarded: an instance without _reader yet (copy, pickle) must not recurse
            raise AttributeError(name)
        return getattr(self._reader, name)

    def get_image_instances(self, idx, *args, **kw):
        out = self._reader.get_image_instances(idx, *args, **kw)
        key = int(idx)
        if key not in self._cache:
            self._cache[key] = RLEMasks.from_dense(out[0])
        return (self._cache[key],) + tuple(out[1:])


def lds_runs():
    """IO_RLE_LDS_RUNS of the built library: the longest run table the decode kernel stages in LDS."""
    return int(_lib.lib().io_rle_lds_runs())


def descriptors(tables, out_offs):
    """(ends uint32, RleDesc array) for ``tables`` = a list of (RLEMasks, instance index) and the byte offset of each
    decoded mask: the run tables of the referenced masks, concatenated."""
    desc = (_lib.RleDesc * len(tables))()
    parts, cursor = [], 0
    for k, ((m, i), o) in enumerate(zip(tables, out_offs)):
        ends, offsets = m.ends()
        a, b = int(offsets[i]), int(offsets[i + 1])
        d = desc[k]
        d.ends_off, d.n_runs, d.H, d.W, d.value, d.out_off = cursor, b - a, m.H, m.W, int(m.values[i]), int(o)
        parts.append(ends[a:b])
        cursor += b - a
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint32)), desc


def group(refs):
    """``arena.Group`` of the run-length instances ``refs`` (the ``tables`` of ``descriptors``): blobs (ends, RleDesc
    array), one ``io_rle_decode_u8`` call, no workspace and no status words"""
    if not refs:
        return arena.Group()
    ends, desc = descriptors(refs, [0] * len(refs))

    def launch(addrs, out, out_bytes, ws, ws_bytes, status, stream, info=None):
        rc = _lib.lib().io_rle_decode_u8(C.c_void_p(addrs[0]), C.c_size_t(ends.size), C.c_void_p(addrs[1]),
                                         C.cast(desc, C.c_void_p), len(desc), C.c_void_p(out), C.c_size_t(out_bytes),
                                         C.c_void_p(stream))
        _lib.check(rc, "io_rle_decode_u8")

    return arena.Group([arena.as_bytes(ends), arena.as_bytes(desc)], ("masks", "descriptors"), desc, launch)


def device_out(who, shape, device, out):
    """the uint8 [n, H, W] device tensor ``rle.decode`` / ``poly.decode`` fill: ``out`` checked, or a new one"""
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=torch.device(device))
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous uint8 device tensor of shape %s" % (who, tuple(shape)))
    return out


def decode(rle_masks, device, out=None):
    """uint8 device tensor [n, H, W] of the masks, through ``io_rle_decode_u8`` (enqueued on the current stream)."""
    _lib.require_gpu()
    n, H, W = rle_masks.shape
    out = device_out("rle.decode", (n, H, W), device, out)
    g = group([(rle_masks, i) for i in range(n)])
    g.set_outs(range(0, n * H * W, H * W))
    arena.decode_into([g], out)
    return out
