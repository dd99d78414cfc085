"""The mask-based order rules of ``inference`` on the device: pair selection ('nbor'), the KINS / COCOA ground truth
(``infer_gt_order``), the area / y-axis baselines and the disparity-selected depth orders of ``midas_pretrained`` and
``InstaDepthNet_d / _od`` with ``disp_select_method``.

The host functions in ``inference`` walk the O(n^2) pairs of an image and redo a full-resolution mask operation per
pair (a cross dilation and an AND in NumPy; a mask upload, two sorts and two syncs for the disparity statistics).  Here
each mask is packed once into a bit image (``io_mask_pack``), every ordered pair is counted in one launch
(``io_mask_pair_counts``), and the per-instance disparity statistics come from exact order statistics
(``io_instance_depth_select``, a fixed number of launches whatever n is).  One copy brings the integers back; the n x n
composition is vectorised NumPy.  Every function returns exactly what its ``inference`` counterpart returns -- those stay
the definition.

Masks: NumPy arrays or device tensors [n, H, W] of bool, an integer type or a float type, with integer values in
0..255 (binary masks, or masks carrying category ids), or ``rle.RLEMasks`` / ``poly.PolyMasks`` (run-length codes and
polygons, decoded on the device).
Anything else raises ValueError before any launch.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, inference
from .rle import is_encoded

MODES = ("host", "device")
_NONZERO, _EQ1 = 0, 1            # IO_MASK_NONZERO, IO_MASK_EQ1
_MEAN, _MEDIAN = 0, 1            # IO_DEPTH_SELECT_MEAN, IO_DEPTH_SELECT_MEDIAN


def check_mode(mask_rules):
    """The ``mask_rules`` keyword of evaluate / inference: 'host' (the per-pair NumPy / torch loops) or 'device'."""
    if mask_rules not in MODES:
        raise ValueError("mask_rules must be 'host' or 'device', got %r" % (mask_rules,))
    return mask_rules == "device"


_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def _check_masks(m, name="masks"):
    """Shape / dtype / value checks: host side for NumPy input, one reduction for a device tensor.  n = 0 is allowed (the
    host functions accept it); an empty image is not.  Encoded masks (``rle.RLEMasks``, ``poly.PolyMasks``) were checked when they were built."""
    if is_encoded(m):
        return
    if torch.is_tensor(m):
        if m.dim() != 3:
            raise ValueError("%s: expected [n, H, W], got shape %s" % (name, tuple(m.shape)))
        if not (m.dtype == torch.bool or m.dtype.is_floating_point or m.dtype in _INT_DTYPES):
            raise ValueError("%s: dtype %s is not bool, integer or float" % (name, m.dtype))
        if m.shape[1] == 0 or m.shape[2] == 0:
            raise ValueError("%s: empty image %s" % (name, tuple(m.shape)))
        if m.dtype in (torch.bool, torch.uint8) or m.shape[0] == 0:
            return
        bad = (m < 0) | (m > 255)
        if m.dtype.is_floating_point:
            bad |= m != torch.trunc(m)          # NaN too
        if bool(bad.any()):
            raise ValueError("%s: values must be integers in 0..255" % name)
        return
    a = np.asarray(m)
    if a.ndim != 3:
        raise ValueError("%s: expected [n, H, W], got shape %s" % (name, a.shape))
    if a.dtype.kind not in ("b", "u", "i", "f"):
        raise ValueError("%s: dtype %s is not bool, integer or float" % (name, a.dtype))
    if a.shape[1] == 0 or a.shape[2] == 0:
        raise ValueError("%s: empty image %s" % (name, a.shape))
    if a.dtype.kind == "b" or a.dtype == np.uint8 or a.shape[0] == 0:
        return
    with np.errstate(invalid="ignore"):
        bad = (a < 0) | (a > 255)
        if a.dtype.kind == "f":
            bad |= a != np.trunc(a)
    if bad.any():
        raise ValueError("%s: values must be integers in 0..255" % name)


def _device(like=None):
    _lib.require_gpu()
    if torch.is_tensor(like) and like.is_cuda:
        return like.device
    return torch.device("cuda", torch.cuda.current_device())


def _to_u8(m, dev):
    """Validated masks -> contiguous uint8 [n, H, W] on ``dev`` (no copy when they already are); run-length and
    polygon masks are decoded there (io_rle_decode_u8, io_poly_fill_u8)."""
    if is_encoded(m):
        return m.to_device(dev)
    if torch.is_tensor(m):
        t = m if m.dtype == torch.uint8 else m.to(torch.uint8)
        return t.to(dev).contiguous()
    a = np.asarray(m)
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8, copy=False))).to(dev)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- device ops ------------------------------------------------------------------------------------------------------
def pack(masks_u8, predicate, dilate=False, stats=None):
    """io_mask_pack: uint8 [n, H, W] device masks -> uint32 bit images [n, H, ceil(W/32)] (enqueued, not synchronised)."""
    n, H, W = masks_u8.shape
    dev = masks_u8.device
    bits = torch.empty((n, H, (W + 31) // 32), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().io_mask_pack(masks_u8.data_ptr(), n, H, W, predicate, 1 if dilate else 0, bits.data_ptr(),
                                       stats.data_ptr() if stats is not None else None, _stream(dev)), "io_mask_pack")
    return bits


def pair_counts(p_bits, q_bits, W, out=None):
    """io_mask_pair_counts: int32 [n_p, n_q] = popcount(P_i & Q_j) over the image (enqueued)."""
    n_p, H, _ = p_bits.shape
    n_q = q_bits.shape[0]
    if out is None:
        out = torch.empty((n_p, n_q), dtype=torch.int32, device=p_bits.device)
    _lib.check(_lib.lib().io_mask_pair_counts(p_bits.data_ptr(), n_p, q_bits.data_ptr(), n_q, H, W, out.data_ptr(),
                                              _stream(p_bits.device)), "io_mask_pair_counts")
    return out


def instance_depth_select(disp, masks_u8, method, out=None):
    """io_instance_depth_select over a device disparity map [H, W] fp32 and uint8 device masks [n, H, W].  Returns the
    device tensors (value, lo, hi) fp32 [n] and k int32 [n] (views of ``out`` when given: fp32 [4, n])."""
    n, H, W = masks_u8.shape
    dev = masks_u8.device
    lib = _lib.lib()
    nws = lib.io_instance_depth_select_workspace_bytes(n, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((4, n), dtype=torch.float32, device=dev)
    kv = out[3].view(torch.int32)
    _lib.check(lib.io_instance_depth_select(disp.data_ptr(), H, W, masks_u8.data_ptr(), n, method, out[0].data_ptr(),
                                            out[1].data_ptr(), out[2].data_ptr(), kv.data_ptr(), ws.data_ptr(), nws,
                                            _stream(dev)), "io_instance_depth_select")
    return out[0], out[1], out[2], kv


# ---- relations -------------------------------------------------------------------------------------------------------
def pair_relations(inmodal, amodal=None):
    """All mask relations of one image from one pack per predicate and one pair-count launch per relation, one copy back.
    Returns a dict of NumPy arrays:
      touch [n, n] bool   = inference.bordering(inmodal[i], inmodal[j]) for every ordered pair (i == j included);
      inter [n, n] int64  = #(inmodal[i] == 1 & amodal[j] == 1)  (only with ``amodal``);
      area [n] = inmodal[i].sum(), n1 [n] = #(inmodal[i] == 1), ysum1 [n] = sum of the row index over inmodal[i] == 1."""
    _check_masks(inmodal, "inmodal")
    if amodal is not None:
        _check_masks(amodal, "amodal")
        if tuple(amodal.shape) != tuple(inmodal.shape):
            raise ValueError("amodal %s and inmodal %s differ in shape" % (tuple(amodal.shape), tuple(inmodal.shape)))
    n = int(inmodal.shape[0])
    if n == 0:
        z = np.zeros(0, np.int64)
        res = {"touch": np.zeros((0, 0), bool), "area": z, "n1": z.copy(), "ysum1": z.copy()}
        if amodal is not None:
            res["inter"] = np.zeros((0, 0), np.int64)
        return res
    dev = _device(inmodal)
    m = _to_u8(inmodal, dev)
    _, H, W = m.shape
    nc = 2 if amodal is not None else 1
    # one buffer for everything that comes back: stats int64 [n, 4], then the int32 count matrices
    buf = torch.empty(8 * n * 4 + 4 * nc * n * n, dtype=torch.uint8, device=dev)
    stats = buf[:32 * n].view(torch.int64).view(n, 4)
    counts = buf[32 * n:].view(torch.int32).view(nc, n, n)
    dil1 = pack(m, _EQ1, dilate=True, stats=stats)
    nz = pack(m, _NONZERO)
    pair_counts(dil1, nz, W, out=counts[0])
    if amodal is not None:
        one = pack(m, _EQ1)
        am1 = pack(_to_u8(amodal, dev), _EQ1)
        pair_counts(one, am1, W, out=counts[1])
    host = buf.cpu().numpy()
    st = host[:32 * n].view(np.int64).reshape(n, 4)
    cn = host[32 * n:].view(np.int32).reshape(nc, n, n)
    res = {"touch": cn[0] > 0, "area": st[:, 0].copy(), "n1": st[:, 1].copy(), "ysum1": st[:, 2].copy()}
    if amodal is not None:
        res["inter"] = cn[1].astype(np.int64)
    return res


def _centre_y(rel):
    with np.errstate(invalid="ignore", divide="ignore"):
        return rel["ysum1"].astype(np.float64) / rel["n1"].astype(np.float64)      # NaN without a '== 1' pixel


def select_pairs(inmodal, pairs):
    """inference.select_pairs on the device ('nbor': one pack + one count launch for all pairs)."""
    if pairs not in ("all", "nbor"):
        raise ValueError("pairs must be 'all' or 'nbor', got %r" % (pairs,))
    _check_masks(inmodal, "inmodal")
    n = int(inmodal.shape[0])
    if pairs == "all":
        return inference.upper_pairs(n)
    touch = pair_relations(inmodal)["touch"]
    ii, jj = np.nonzero(np.triu(touch, 1))
    return [(int(i), int(j)) for i, j in zip(ii, jj)]           # row-major: the order of the host double loop


def _pairwise(n, keys, touch, direction):
    """inference._pairwise on the n x n keys: for i < j (only where ``touch``, if given) lo = i if keys[i] < keys[j]
    else j (strict <, NaN compares false), [lo, hi] = 1 if ``direction`` else [hi, lo] = 1."""
    sel = np.triu(np.ones((n, n), dtype=bool), 1)
    if touch is not None:
        sel &= touch
    with np.errstate(invalid="ignore"):
        less = keys[:, None] < keys[None, :]
    order = np.zeros((n, n), dtype=np.int64)
    order[sel & (less == direction)] = 1                  # mark [i, j]
    order[(sel & (less != direction)).T] = 1              # mark [j, i]
    return order


def infer_occ_order_area(inmodal, occluder="smaller"):
    r = pair_relations(inmodal)
    return _pairwise(len(r["area"]), r["area"], r["touch"], occluder == "smaller")


def infer_occ_order_yaxis(inmodal, occluder="lower"):
    r = pair_relations(inmodal)
    return _pairwise(len(r["area"]), _centre_y(r), r["touch"], occluder == "lower")


def infer_depth_order_area(inmodal, closer="smaller"):
    r = pair_relations(inmodal)
    return _pairwise(len(r["area"]), r["area"], None, closer == "smaller")


def infer_depth_order_yaxis(inmodal, closer="lower"):
    r = pair_relations(inmodal)
    return _pairwise(len(r["area"]), _centre_y(r), None, closer != "lower")


def infer_gt_order(inmodal, amodal):
    """inference.infer_gt_order: for bordering i < j with a non-empty overlap, i occludes j when
    #(inmodal_i == 1 & amodal_j == 1) >= #(inmodal_j == 1 & amodal_i == 1)."""
    r = pair_relations(inmodal, amodal)
    n = len(r["area"])
    inter = r["inter"]
    sel = np.triu(r["touch"], 1) & ((inter != 0) | (inter.T != 0))
    ge = inter >= inter.T
    gt = np.zeros((n, n), dtype=np.int64)
    gt[sel & ge] = 1
    gt[(sel & ~ge).T] = 1
    return gt


# ---- disparity-selected depth orders --------------------------------------------------------------------------------
def depth_orders_from_disp(disp, masks, pair_list, disp_select_method):
    """The order matrix of the host loop over ``pair_list`` with ``inference.net_forward_midas_pretrained``: [i, j] / [j, i]
    = 1 / 0 when instance i's statistic is smaller, 0 / 1 when larger, 2 / 2 when equal or NaN.  ``disp``: the disparity
    map [H, W] (any leading singleton dims) on the device; ``masks`` [n, H, W] (instance i = masks[i] != 0).  One
    io_instance_depth_select, one copy back.  An empty instance inside a selected pair raises RuntimeError (as
    torch.quantile does on the host path)."""
    _check_masks(masks, "masks")
    n, H, W = (int(v) for v in masks.shape)
    if not torch.is_tensor(disp) or disp.numel() != H * W:
        raise ValueError("disp: expected a tensor of %d x %d values" % (H, W))
    pair_list = [(int(i), int(j)) for i, j in pair_list]
    for i, j in pair_list:
        if not (0 <= i < n and 0 <= j < n):
            raise ValueError("pair (%d, %d) outside 0..%d" % (i, j, n - 1))
    order = np.zeros((n, n), dtype=np.int64)
    if n == 0:
        return order
    dev = _device(disp if disp.is_cuda else masks)
    d = disp.detach().reshape(H, W).to(dev, torch.float32).contiguous()
    m = _to_u8(masks, dev)
    method = _MEDIAN if disp_select_method == "median" else _MEAN
    out = torch.empty((4, n), dtype=torch.float32, device=dev)
    instance_depth_select(d, m, method, out=out)
    host = out.cpu().numpy()
    val, k = host[0], host[3].view(np.int32)
    if not pair_list:
        return order
    ii = np.array([p[0] for p in pair_list], np.int64)
    jj = np.array([p[1] for p in pair_list], np.int64)
    empty = (k[ii] == 0) | (k[jj] == 0)
    if empty.any():
        q = int(np.nonzero(empty)[0][0])
        raise RuntimeError("depth_orders_from_disp: pair (%d, %d) has an empty mask (torch.quantile() needs a non-empty "
                           "input)" % (ii[q], jj[q]))
    a, b = val[ii], val[jj]
    closer, farther = a < b, a > b
    order[ii, jj] = np.where(closer, 1, np.where(farther, 0, 2))
    order[jj, ii] = np.where(closer, 0, np.where(farther, 1, 2))
    return order
