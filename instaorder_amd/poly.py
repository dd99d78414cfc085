"""COCO polygon instance masks for the device input pipeline.

A non-crowd COCO annotation (InstaOrder, COCOA) stores ``segmentation`` as a list of polygons; the reference rasterises
them on the host (``maskUtils.frPyObjects`` + ``maskUtils.merge``, datasets/reader.py:31-46).  Here the vertices travel to
the GPU -- a few dozen int32 pairs per instance instead of H * W bytes -- and ``io_poly_fill_u8`` (csrc/poly.hip) fills
them there, next to ``io_rle_decode_u8``, in front of the render kernel (``datasets.PairRenderer``) and of the mask rules.
``PolyMasks`` holds the instances of one image; since a COCO image mixes polygons with run-length codes (its crowd
regions), an instance may be either.

The fill rule is the published COCO mask API's, restated (DESIGN.md "Polygon masks"); one polygon part is k >= 1 vertices:

1. Scale: X = trunc(5 x + 0.5), Y = trunc(5 y + 0.5) in double, truncating toward zero; the ring closes on vertex 0.
2. Walk every edge in max(dx, dy) unit steps along its longer axis, from the end with the smaller major coordinate; the
   minor coordinate of step t is trunc(b + s * t + 0.5) with the slope s = (difference of the minor ends) / max(dx, dy),
   product and sums rounded separately.
3. Two consecutive walk points with different X are a crossing: with c the larger X and Ymin the smaller Y it counts if
   c = 5 x + 3 for a column 0 <= x < W, at row y = ceil(clamp((Ymin + 0.5) / 5 - 0.5, 0, H)), position a = x * H + y.
4. Pixel q = x * H + y (column-major) of the part is set iff the number of positions a <= q is odd.
5. An instance is the OR of its parts; an instance without parts is empty.

``to_dense()`` is that rule in NumPy; the kernel is the same rule on bit planes.  Neither could be compared with a
pycocotools binary where this was written; tests/test_poly_cpu.py holds fixed vectors derived from the text.
"""
import ctypes as C
import numbers

import numpy as np

from . import _lib, arena
from . import rle as _rle
from .rle import EncodedMasks, RLEMasks

SCALE = 5
MAX_SCALED = 1 << 24            # IO_POLY_MAX_COORD: |5 * coordinate| above it is refused (the kernel would clamp)


def _scaled_part(flat, where):
    """flat [x0, y0, x1, y1, ...] -> int32 [k, 2] of step 1"""
    a = np.asarray(flat, dtype=np.float64)
    if a.ndim != 1 or a.size < 2 or a.size % 2:
        raise ValueError("PolyMasks: %s: a part is a flat sequence x0, y0, x1, y1, ... of even length >= 2 (got shape %s)"
                         % (where, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("PolyMasks: %s has a coordinate that is not finite" % where)
    if (np.abs(a) * SCALE > MAX_SCALED).any():
        raise ValueError("PolyMasks: %s has a coordinate beyond +-%d / %d" % (where, MAX_SCALED, SCALE))
    return np.trunc(SCALE * a + 0.5).astype(np.int32).reshape(-1, 2)


def _part_positions(V, H, W):
    """Steps 2 and 3 for one part: the positions a of its crossings (int64, in no particular order)."""
    k = V.shape[0]
    found = []
    for j in range(k):
        (xs, ys), (xe, ye) = (int(c) for c in V[j]), (int(c) for c in V[(j + 1) % k])
        dx, dy = abs(xe - xs), abs(ye - ys)
        n = max(dx, dy)
        if n == 0:
            continue
        flat = dx >= dy
        if (xs > xe) if flat else (ys > ye):
            xs, ys, xe, ye = xe, ye, xs, ys
        t = np.arange(n + 1, dtype=np.int64)
        tf = t.astype(np.float64)
        if flat:
            s = np.float64(ye - ys) / np.float64(dx)
            u = xs + t
            v = np.trunc((np.float64(ys) + s * tf) + 0.5).astype(np.int64)
        else:
            s = np.float64(xe - xs) / np.float64(dy)
            v = ys + t
            u = np.trunc((np.float64(xs) + s * tf) + 0.5).astype(np.int64)
        # a crossing is a property of two neighbouring walk points, so the direction of the walk does not enter
        c = np.maximum(u[1:], u[:-1])
        vmin = np.minimum(v[1:], v[:-1])
        x = (c - 3) // SCALE
        ok = (u[1:] != u[:-1]) & ((c - 3) % SCALE == 0) & (x >= 0) & (x <= W - 1)
        yd = (vmin[ok].astype(np.float64) + 0.5) / SCALE - 0.5
        y = np.ceil(np.clip(yd, 0.0, float(H))).astype(np.int64)
        found.append(x[ok] * H + y)
    return np.concatenate(found) if found else np.zeros(0, np.int64)


def _fill(positions, H, W):
    """Step 4: bool [H, W] from the positions of one part."""
    a = positions[positions < H * W]
    toggles = np.bincount(a, minlength=H * W)
    return (np.cumsum(toggles) & 1).astype(bool).reshape(W, H).T


def _is_scalar(v):
    return isinstance(v, (numbers.Number, np.generic))


def _rle_counts(obj, H, W, where):
    """a run-length instance -> counts: a COCO RLE dict (counts as list / str / bytes) or the counts themselves"""
    if isinstance(obj, dict):
        if "size" in obj and tuple(int(v) for v in obj["size"]) != (H, W):
            raise ValueError("PolyMasks: %s has size %s, the image %s" % (where, list(obj["size"]), [H, W]))
        obj = obj["counts"]
        if isinstance(obj, (str, bytes)):
            obj = _rle._counts_from_string(obj)
    return np.asarray(obj)


class PolyMasks(EncodedMasks):
    """The n instance masks of one image, each a list of polygon parts (flat ``[x0, y0, x1, y1, ...]`` sequences, image
    coordinates) or a run-length code (a COCO RLE dict, or its counts as a flat integer sequence); ``values`` is the byte
    each mask carries where it is set (1, or a category id).  Stands in for a uint8 [n, H, W] array wherever
    ``rle.RLEMasks`` does."""

    def __init__(self, segmentations, H, W, values=None):
        H, W = int(H), int(W)
        if H <= 0 or W <= 0 or H * W >= 1 << 31:
            raise ValueError("PolyMasks: size %d x %d (need H, W > 0 and H * W < 2^31)" % (H, W))
        inst = []
        for i, seg in enumerate(segmentations):
            where = "instance %d" % i
            if isinstance(seg, dict) or (isinstance(seg, np.ndarray) and seg.ndim == 1 and seg.size
                                         and seg.dtype.kind in ("u", "i")):
                inst.append(RLEMasks([_rle_counts(seg, H, W, where)], H, W))
                continue
            parts = list(seg)
            if parts and all(_is_scalar(p) for p in parts):
                if not all(isinstance(p, (numbers.Integral, np.integer)) for p in parts):
                    raise ValueError("PolyMasks: %s is a flat sequence of floats: an instance is a LIST of parts "
                                     "(wrap a single polygon in a list)" % where)
                inst.append(RLEMasks([np.asarray(parts)], H, W))
                continue
            inst.append([_scaled_part(p, "%s part %d" % (where, k)) for k, p in enumerate(parts)])
        self._inst = inst
        self.H, self.W = H, W
        self.values = self._check_values(values, len(inst), "PolyMasks")
        self._sync_rle()

    @staticmethod
    def _check_values(values, n, who):
        if values is None:
            return np.ones(n, np.int64)
        v = np.asarray(values)
        if v.dtype.kind not in ("u", "i", "b"):
            raise ValueError("%s: integer values expected (got %s)" % (who, v.dtype))
        v = np.broadcast_to(v.astype(np.int64), (n,)).copy()
        if n and (v.min() < 0 or v.max() > 255):
            raise ValueError("%s: values must lie in 0..255" % who)
        return v

    def _sync_rle(self):
        """the run-length instances carry their value themselves (``rle.descriptors`` reads it there)"""
        for i, e in enumerate(self._inst):
            if isinstance(e, RLEMasks) and int(e.values[0]) != int(self.values[i]):
                e.ends()                                         # computed once, shared by the copy
                self._inst[i] = e.with_values(int(self.values[i]))

    def _like(self, inst, values):
        out = PolyMasks.__new__(PolyMasks)
        out._inst = list(inst)
        out.H, out.W = self.H, self.W
        out.values = values
        out._sync_rle()
        return out

    # ---- the part of the array interface the consumers use ----------------------------------------------------------
    @property
    def shape(self):
        return (len(self._inst), self.H, self.W)

    def __len__(self):
        return len(self._inst)

    def is_polygon(self, i):
        return not isinstance(self._inst[i], RLEMasks)

    def parts(self, i):
        """the scaled vertices (int32 [k, 2] per part) of polygon instance i"""
        if not self.is_polygon(i):
            raise ValueError("PolyMasks: instance %d is a run-length code" % i)
        return self._inst[i]

    def rle_ref(self, i):
        """(RLEMasks, 0) for the run-length instance i -- an entry of ``rle.descriptors`` -- or None for a polygon"""
        return None if self.is_polygon(i) else (self._inst[i], 0)

    def __getitem__(self, idx):
        """Instances by index: an int gives the one-mask PolyMasks (shape (1, H, W)), a list / array / slice the subset."""
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
                raise IndexError("PolyMasks are indexed by instance: an int, a slice or a 1-D list of ints")
        return self._like([self._inst[i] for i in sel],
                          self.values[[int(i) for i in sel]] if sel else np.zeros(0, np.int64))

    def with_values(self, category):
        """The same masks carrying ``category`` (a scalar or one id per mask) where they are set.  Shares the vertices."""
        return self._like(self._inst, self._check_values(category, len(self), "PolyMasks.with_values"))

    def to_dense(self):
        """uint8 [n, H, W] on the host, by the rule of the module docstring (what host-only code paths use)."""
        n, H, W = self.shape
        out = np.zeros((n, H, W), np.uint8)
        for i, e in enumerate(self._inst):
            if isinstance(e, RLEMasks):
                out[i] = e.to_dense()[0]
                continue
            m = np.zeros((H, W), bool)
            for V in e:
                m |= _fill(_part_positions(V, H, W), H, W)
            out[i] = m * np.uint8(self.values[i])
        return out

    def to_device(self, device, out=None):
        return decode(self, device, out=out)

    @classmethod
    def from_coco(cls, anns_or_segmentations, H, W, values=None):
        """From the annotations of one image, or their ``segmentation`` fields, in the three forms ``read_LVIS`` meets: a
        list of polygons, and a run-length dict whose ``counts`` is a list or a compressed string / bytes."""
        segs = []
        for i, a in enumerate(anns_or_segmentations):
            if isinstance(a, dict) and "segmentation" in a:
                a = a["segmentation"]
            if isinstance(a, dict):
                if "counts" not in a:
                    raise ValueError("PolyMasks.from_coco: object %d is a dict without 'counts'" % i)
            elif not isinstance(a, (list, tuple)):
                raise ValueError("PolyMasks.from_coco: object %d is neither a polygon list nor a run-length dict" % i)
            elif a and all(_is_scalar(p) for p in a):
                raise ValueError("PolyMasks.from_coco: object %d is a flat list, not a list of polygons" % i)
            segs.append(a)
        return cls(segs, H, W, values=values)


def scan_words():
    """IO_POLY_SCAN_WORDS of the built library: the 32-bit words of a bit plane one pass of the parity scan covers."""
    return int(_lib.lib().io_poly_scan_words())


def descriptors(tables, out_offs):
    """(verts int32 [nv, 2], PolyPart array, PolyMask array, n_parts) for ``tables`` = a list of (PolyMasks, index of a
    POLYGON instance) and the byte offset of each filled mask: what ``io_poly_fill_u8`` reads.  (The part array has one
    unused entry when n_parts is 0: ctypes arrays of length 0 have no address.)"""
    n_parts = sum(len(m.parts(i)) for m, i in tables)
    parts = (_lib.PolyPart * max(n_parts, 1))()
    masks = (_lib.PolyMask * len(tables))()
    verts, p, cursor = [], 0, 0
    for k, ((m, i), o) in enumerate(zip(tables, out_offs)):
        d = masks[k]
        d.H, d.W, d.value, d.first_part, d.n_parts, d.out_off = m.H, m.W, int(m.values[i]), p, len(m.parts(i)), int(o)
        for V in m.parts(i):
            parts[p].vert_off, parts[p].n_verts, parts[p].mask = cursor, V.shape[0], k
            verts.append(V)
            cursor += V.shape[0]
            p += 1
    v = np.ascontiguousarray(np.concatenate(verts)) if verts else np.zeros((0, 2), np.int32)
    return v, parts, masks, n_parts


def workspace_bytes(parts, n_parts, masks):
    b = int(_lib.lib().io_poly_fill_workspace_bytes(C.cast(parts, C.c_void_p), n_parts, C.cast(masks, C.c_void_p), len(masks)))
    if b == 0:
        raise RuntimeError("instaorder_hip io_poly_fill_workspace_bytes refused the tables: %s" % _lib.last_error())
    return b


def group(refs):
    """``arena.Group`` of the polygon instances ``refs`` (the ``tables`` of ``descriptors``): blobs (vertices, PolyPart
    array, PolyMask array), one ``io_poly_fill_u8`` call with a workspace, no status words"""
    if not refs:
        return arena.Group()
    verts, parts, masks, n_parts = descriptors(refs, [0] * len(refs))

    def launch(addrs, out, out_bytes, ws, ws_bytes, status, stream, info=None):
        rc = _lib.lib().io_poly_fill_u8(C.c_void_p(addrs[0]), C.c_size_t(verts.shape[0]), C.c_void_p(addrs[1]),
                                        C.cast(parts, C.c_void_p), n_parts, C.c_void_p(addrs[2]), C.cast(masks, C.c_void_p),
                                        len(masks), C.c_void_p(out), C.c_size_t(out_bytes), C.c_void_p(ws),
                                        C.c_size_t(ws_bytes), C.c_void_p(stream))
        _lib.check(rc, "io_poly_fill_u8")

    return arena.Group([arena.as_bytes(verts), arena.as_bytes(parts), arena.as_bytes(masks)],
                       ("masks", "descriptors", "descriptors"), masks, launch,
                       lambda: workspace_bytes(parts, n_parts, masks))


def decode(poly_masks, device, out=None):
    """uint8 device tensor [n, H, W] of the masks: the polygon instances through ``io_poly_fill_u8``, the run-length ones
    through ``io_rle_decode_u8`` (both enqueued on the current stream)."""
    _lib.require_gpu()
    n, H, W = poly_masks.shape
    out = _rle.device_out("poly.decode", (n, H, W), device, out)
    pol = [i for i in range(n) if poly_masks.is_polygon(i)]
    enc = [i for i in range(n) if not poly_masks.is_polygon(i)]
    groups = [group([(poly_masks, i) for i in pol]), _rle.group([poly_masks.rle_ref(i) for i in enc])]
    groups[0].set_outs(i * H * W for i in pol)
    groups[1].set_outs(i * H * W for i in enc)
    arena.decode_into(groups, out)
    return out
