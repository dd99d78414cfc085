"""Dense-disparity evaluation of the MiDaS nets: the reference's ``tools/test_disp_KITTI.py`` (Eigen-split depth errors of
the predicted disparity, "median" conversion) and ``tools/test_disp_DIW.py`` (ordinal WHDR of the disparity at the
annotated point pairs), batched.

The reference evaluates one image at a time and computes its metrics in NumPy after a ``.cpu()``.  Here images are
decoded on a worker thread, rendered by the device pre-processing kernel (``io_pair_planes_u8_hw``) on a side stream,
run through the net's encoder + decoder only (the disparity does not depend on the masks the reference feeds as zeros),
and the metrics are computed on the device (``io_depth_errors_median``, ``io_disp_sample_points``).  Per-image rows stay
on the device until the end of the run and are read back once.  With ``world_size > 1`` each rank takes a contiguous
slice (``distributed_utils.shard_range``) and the rows are gathered as in ``evaluate``.

Not reproduced: the 'nyu' branch of test_disp_KITTI.py (broken in the reference), the unused 'scale-shift' conversion,
png / histogram dumps and wandb.
"""
import csv
import ctypes as C
import os
import queue
import threading

import numpy as np
import torch

from . import _lib

KITTI_H, KITTI_W = 352, 1216
DIW_SIZE = 384
ERROR_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "silog")
ROW_WIDTH = 10          # ERROR_NAMES + n_valid + ratio
_INTER_LINEAR = 1


def _stream_ptr(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- device ops ------------------------------------------------------------------------------------------------------
def depth_errors_median(pred, gt, gt_div=256.0, min_depth=1e-3, max_depth=80.0, out=None, medians=None):
    """pred [B,H,W] fp32 disparity, gt [B,H,W] raw uint16 ground truth (torch.uint16 or its int16 view) on the GPU.
    Returns the fp64 rows [B,10] (``ERROR_NAMES``, n_valid, ratio) on the device, enqueued on the current stream;
    ``medians`` (optional fp32 [B,2] device tensor) receives median(gt[valid]), median(depth[valid])."""
    if pred.dim() != 3 or gt.shape != pred.shape:
        raise ValueError("pred %s / gt %s: expected two [B,H,W] tensors" % (tuple(pred.shape), tuple(gt.shape)))
    if pred.dtype != torch.float32 or gt.dtype not in (torch.int16, torch.uint16) or not pred.is_cuda or not gt.is_cuda:
        raise TypeError("pred must be fp32 and gt uint16 / int16, both on the GPU")
    pred, gt = pred.contiguous(), gt.contiguous()
    B, H, W = pred.shape
    lib = _lib.lib()
    nws = lib.io_depth_errors_median_workspace_bytes(B, H, W)
    ws = torch.empty(nws, dtype=torch.uint8, device=pred.device)
    if out is None:
        out = torch.empty((B, ROW_WIDTH), dtype=torch.float64, device=pred.device)
    _lib.check(lib.io_depth_errors_median(pred.data_ptr(), gt.data_ptr(), B, H, W, gt_div, min_depth, max_depth,
                                          out.data_ptr(), medians.data_ptr() if medians is not None else None,
                                          ws.data_ptr(), nws, _stream_ptr(pred.device)),
               "io_depth_errors_median")
    return out


def disp_sample_points(disp, points):
    """disp [B,H,W] fp32, points [B,6] int32 (h, w, Ay, Ax, By, Bx) on the GPU -> (values [B,2] fp32, decisions [B] int32:
    ord('<') if dA > dB, ord('>') if dA < dB, ord('=') if equal), as F.interpolate(size=(h, w), mode='bilinear',
    align_corners=False)[Ay, Ax] / [By, Bx] without the upsampled map."""
    if disp.dim() != 3 or disp.dtype != torch.float32 or not disp.is_cuda:
        raise TypeError("disp must be an fp32 [B,H,W] GPU tensor")
    B, H, W = disp.shape
    points = points.to(disp.device, torch.int32).contiguous()
    if tuple(points.shape) != (B, 6):
        raise ValueError("points: expected [%d,6], got %s" % (B, tuple(points.shape)))
    disp = disp.contiguous()
    vals = torch.empty((B, 2), dtype=torch.float32, device=disp.device)
    dec = torch.empty((B,), dtype=torch.int32, device=disp.device)
    _lib.check(_lib.lib().io_disp_sample_points(disp.data_ptr(), B, H, W, points.data_ptr(), vals.data_ptr(),
                                                dec.data_ptr(), _stream_ptr(disp.device)), "io_disp_sample_points")
    return vals, dec


# ---- readers ---------------------------------------------------------------------------------------------------------
def _read_rgb(path):
    from PIL import Image
    return np.array(Image.open(path).convert("RGB"))


def _read_png16(path):
    """cv2.imread(path, -1) of a 16-bit PNG (same uint16 values), or None when the file is missing."""
    if not os.path.isfile(path):
        return None
    from PIL import Image
    a = np.array(Image.open(path))
    return a.astype(np.uint16) if a.dtype != np.uint16 else a


def _device_png(path, raw16):
    """the file as a ``png.PngImage`` when the device decoder takes it in the wanted form (8-bit picture, or 16-bit
    grayscale with ``raw16``), else None: the caller reads it on the host"""
    from . import png
    try:
        im = png.PngImage.open(path)
    except ValueError:
        return None
    return im if im.supported and im.raw16 == raw16 else None


def kitti_crop_box(H, W):
    """datasets/reader.py:83-85: the bottom 352 rows, 1216 columns starting at int((W - 1216) / 2) -> (x, y, w, h)."""
    if H < KITTI_H or W < KITTI_W:
        raise ValueError("KITTI image %dx%d is smaller than the %dx%d crop" % (H, W, KITTI_H, KITTI_W))
    return int((W - KITTI_W) / 2), int(H - KITTI_H), KITTI_W, KITTI_H


class KITTIEigenReader(object):
    """datasets/reader.py:69-96 KITTIDataset: list lines ``image depth [focal]``; images under ``<root>/rawdata/``, 16-bit
    ground truth under ``<root>/data_depth_annotated/``.  A ground truth that does not exist (the Eigen list names
    ``None`` for some images) is reported by ``has_gt``.  ``png="device"``: ``load`` returns the frame and the ground truth
    as ``png.PngImage`` objects (the ground truth whole, in the raw16 form) for ``io_png_decode``; a file that is not in a
    form the device decoder takes comes as the array of the default ``"host"`` path.  ``png=None`` (the default) takes the
    environment variable IO_KITTI_PNG, "host" when it is unset or empty: the switch of ``tools/test_disp.py``, which builds
    its reader without the argument.  Any other value, from either source, raises ValueError."""

    def __init__(self, list_file, root, test_num=-1, png=None):
        if png is None:
            png = os.environ.get("IO_KITTI_PNG", "") or "host"
        if png not in ("host", "device"):
            raise ValueError("KITTIEigenReader: png %r ('host' or 'device'; IO_KITTI_PNG when not given)" % (png,))
        self.png = png
        with open(list_file, "r") as f:
            lines = [ln.split() for ln in f.readlines()]
        lines = [ln for ln in lines if ln]
        if test_num is not None and test_num > 0:
            lines = lines[:test_num]
        self.image_paths = [os.path.join("%s/rawdata/%s" % (root, ln[0])) for ln in lines]
        self.depth_paths = [os.path.join("%s/data_depth_annotated/%s" % (root, ln[1])) for ln in lines]

    def __len__(self):
        return len(self.image_paths)

    def has_gt(self, i):
        return os.path.isfile(self.depth_paths[i])

    def load(self, i):
        """-> (uint8 image [H,W,3], crop box (x, y, w, h), raw uint16 ground truth cropped to [352,1216] or None); with
        ``png="device"`` the image and the (uncropped) ground truth may be ``png.PngImage`` objects."""
        img = _device_png(self.image_paths[i], False) if self.png == "device" else None
        if img is None:
            img = _read_rgb(self.image_paths[i])
        box = kitti_crop_box(img.shape[0], img.shape[1])
        gt = None
        if self.png == "device" and os.path.isfile(self.depth_paths[i]):
            gt = _device_png(self.depth_paths[i], True)
            if gt is not None:
                kitti_crop_box(gt.H, gt.W)
                return img, box, gt
        gt = _read_png16(self.depth_paths[i])
        if gt is not None:
            x, y, w, h = kitti_crop_box(gt.shape[0], gt.shape[1])
            gt = np.ascontiguousarray(gt[y:y + h, x:x + w])
        return img, box, gt


class DIWReader(object):
    """datasets/reader.py:126-199 DIWDataset: a CSV of an image line (``./DIW_test/xxx.thumb``, resolved under ``root``)
    followed by a point line ``A_y, A_x, B_y, B_x, ordinal, ...`` with 1-based points; the ordinal is the first character
    of field 4.  Images are converted to RGB (so the reference's grayscale float64 branch never runs)."""

    def __init__(self, csv_file, root, test_num=-1):
        with open(csv_file, "r") as f:
            rows = list(csv.reader(f))
        self.image_paths, self.points, self.ordinals = [], [], []
        for k in range(0, len(rows) - 1, 2):
            fn, pt = rows[k][0], rows[k + 1]
            self.image_paths.append("%s/%s" % (root, fn[1:]))
            self.points.append(tuple(int(pt[j]) - 1 for j in range(4)))       # A_y, A_x, B_y, B_x, 0-based
            self.ordinals.append(pt[4][0])
        if test_num is not None and test_num > 0:
            self.image_paths, self.points, self.ordinals = (self.image_paths[:test_num], self.points[:test_num],
                                                            self.ordinals[:test_num])

    def __len__(self):
        return len(self.image_paths)

    def load(self, i):
        """-> (uint8 image [h,w,3], (A_y, A_x, B_y, B_x), ordinal character)."""
        img = _read_rgb(self.image_paths[i])
        h, w = img.shape[:2]
        ay, ax, by, bx = self.points[i]
        for y, x in ((ay, ax), (by, bx)):
            if not (0 <= y < h and 0 <= x < w):
                raise ValueError("%s: point (%d, %d) outside the %dx%d image" % (self.image_paths[i], y, x, h, w))
        return img, self.points[i], self.ordinals[i]


# ---- batching --------------------------------------------------------------------------------------------------------
class _Prefetch(object):
    """Runs ``make(indices)`` for each batch on a worker thread (image decode + upload + render on a side stream), as
    datasets.BatchPrefetcher does for training; yields (tensors, meta) with the consumer stream ordered after the render."""

    def __init__(self, make, index_batches, device, depth=2):
        self._q = queue.Queue(maxsize=depth)
        self._stream = torch.cuda.Stream(device=device)
        self._device = device
        self._err = None
        self._stop = False

        def work():
            try:
                with torch.cuda.stream(self._stream):
                    for idx in index_batches:
                        if self._stop:
                            break
                        tensors, meta = make(idx)
                        ev = torch.cuda.Event()
                        ev.record(self._stream)
                        self._q.put((tensors, meta, ev))
            except BaseException as e:          # surfaced on the consumer side
                self._err = e
            self._q.put(None)

        self._thread = threading.Thread(target=work, daemon=True)
        self._thread.start()

    def __iter__(self):
        while True:
            item = self._q.get()
            if item is None:
                if self._err is not None:
                    raise self._err
                return
            tensors, meta, ev = item
            cur = torch.cuda.current_stream(self._device)
            cur.wait_event(ev)
            for t in tensors:
                t.record_stream(cur)
            yield tensors, meta

    def close(self):
        self._stop = True
        while self._thread.is_alive():
            try:
                self._q.get(timeout=0.1)
            except queue.Empty:
                pass


def _renderer(size, mean, std, device):
    from .datasets import PairRenderer
    return PairRenderer(size, mean, std, device=device)


def render_rgb(renderer, images, boxes):
    """uint8 images + crop boxes -> normalised rgb [P,3,SH,S] through io_pair_planes_u8_hw (INTER_LINEAR; a box of the
    output's size is an exact crop).  One shared all-zero mask per image stands in for the instance masks."""
    masks = [np.zeros((1,) + im.shape[:2], np.uint8) for im in images]
    items = [(k, 0, 0, box, _INTER_LINEAR, False) for k, box in enumerate(boxes)]
    rgb, _, _ = renderer.render(images, masks, items)
    return rgb


def _disparity_net(model, algo):
    if algo == "midas_pretrained":
        return model
    if algo in ("InstaDepthNet_d", "InstaDepthNet_od"):
        return model.net
    raise Exception("No such algo for dense evaluation: {}".format(algo))


def _shard(n, world_size, rank):
    if world_size <= 1:
        return list(range(n))
    from .distributed_utils import shard_range
    beg, end, _ = shard_range(n, world_size, rank)
    return [q % n for q in range(beg, end)]


def _disparity(net, rgb):
    with torch.no_grad():
        disp, _ = net._encode_decode(rgb)
    return disp.reshape(rgb.shape[0], rgb.shape[2], rgb.shape[3]).float()


def _collect(chunks, n, world_size):
    """[(indices, device rows)] -> [n, width] table on every rank (one device -> host copy)."""
    from .evaluate import _gather_rows
    rows = {}
    if chunks:
        allrows = torch.cat([r for _, r in chunks], 0).cpu().numpy()
        k = 0
        for idx, r in chunks:
            for j, i in enumerate(idx):
                rows[i] = allrows[k + j]
            k += r.shape[0]
    return _gather_rows(rows, n, world_size)


# ---- drivers ---------------------------------------------------------------------------------------------------------
def eval_dense_depth(model, reader, algo, batch=4, min_depth=1e-3, max_depth=80, world_size=1, rank=0,
                     data_mean=(0.485, 0.456, 0.406), data_std=(0.229, 0.224, 0.225), device="cuda", return_rows=False):
    """test_disp_KITTI.py:eval_dense_depth ('kitti', 'median') over ``reader`` (KITTIEigenReader).  Returns a dict with the
    eight means over the evaluated images (NumPy ``.mean(0)``), ``n_images`` and ``missing`` (images without ground
    truth: skipped); with ``return_rows`` also ``rows`` [n_images, 10] (ERROR_NAMES, n_valid, ratio)."""
    net = _disparity_net(model, algo)
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    n = len(reader)
    present = [i for i in range(n) if reader.has_gt(i)]
    missing = n - len(present)
    mine = [i for i in _shard(len(present), world_size, rank)]
    ren = _renderer((KITTI_H, KITTI_W), data_mean, data_std, dev)
    from . import png

    def make(ks):
        imgs, boxes, gts = [], [], []
        for k in ks:
            img, box, gt = reader.load(present[k])
            if gt is None:
                raise RuntimeError("ground truth of %s disappeared" % reader.image_paths[present[k]])
            if not png.is_png(gt) and gt.shape != (KITTI_H, KITTI_W):
                raise ValueError("ground truth %s: crop %s" % (reader.depth_paths[present[k]], gt.shape))
            imgs.append(img)
            boxes.append(box)
            gts.append(gt)
        rgb = render_rgb(ren, imgs, boxes)
        on_dev = [j for j, gt in enumerate(gts) if png.is_png(gt)]
        if not on_dev:
            g = torch.from_numpy(np.stack(gts).view(np.int16)).pin_memory().to(dev, non_blocking=True)
            return (rgb, g), list(ks)
        # ground truth that arrived as PNG files: one decode for the batch on this (the prefetch) stream, cropped on the device
        g = torch.empty((len(gts), KITTI_H, KITTI_W), dtype=torch.int16, device=dev)
        maps = png.decode([gts[j] for j in on_dev], dev)
        for j, m in zip(on_dev, maps):
            x, y, w, h = kitti_crop_box(m.shape[0], m.shape[1])
            g[j].copy_(m.view(torch.int16)[y:y + h, x:x + w])
        for j, gt in enumerate(gts):
            if not png.is_png(gt):
                g[j].copy_(torch.from_numpy(gt.view(np.int16)).pin_memory(), non_blocking=True)
        return (rgb, g), list(ks)

    chunks = []
    pf = _Prefetch(make, [mine[s:s + batch] for s in range(0, len(mine), batch)], dev)
    try:
        for (rgb, g), ks in pf:
            disp = _disparity(net, rgb)
            chunks.append((ks, depth_errors_median(disp, g, 256.0, min_depth, max_depth)))
    finally:
        pf.close()
    ren.check_status()                                       # a PNG frame of the last batches that did not decode
    table = _collect(chunks, len(present), world_size)
    out = {}
    means = table[:, :8].mean(0) if len(present) else np.full(8, np.nan)
    for k, name in enumerate(ERROR_NAMES):
        out[name] = float(means[k])
    out["n_images"] = len(present)
    out["missing"] = missing
    if return_rows:
        out["rows"] = table
    return out


def eval_ordinal_via_disp(model, reader, algo, batch=8, world_size=1, rank=0, data_mean=(0.485, 0.456, 0.406),
                          data_std=(0.229, 0.224, 0.225), device="cuda", return_decisions=False):
    """test_disp_DIW.py:eval_ordinal_via_disp over ``reader`` (DIWReader): the disparity of the 384x384 input, bilinearly
    resized to the thumbnail's size, compared at the two points ('<' if dA > dB, '>' if dA < dB, '=' if equal) against
    the annotated ordinal.  Returns dict(WHDR = wrong / total * 100, wrong, total); with ``return_decisions`` also
    ``decisions``: the predicted ordinal characters in reader order."""
    net = _disparity_net(model, algo)
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    n = len(reader)
    mine = _shard(n, world_size, rank)
    ren = _renderer(DIW_SIZE, data_mean, data_std, dev)

    def make(ks):
        imgs, pts, gts = [], [], []
        for k in ks:
            img, (ay, ax, by, bx), o = reader.load(k)
            imgs.append(img)
            pts.append((img.shape[0], img.shape[1], ay, ax, by, bx))
            gts.append(ord(o))
        rgb = render_rgb(ren, imgs, [(0, 0, im.shape[1], im.shape[0]) for im in imgs])
        meta = torch.tensor(np.concatenate([np.asarray(pts, np.int32), np.asarray(gts, np.int32)[:, None]], 1))
        return (rgb, meta.pin_memory().to(dev, non_blocking=True)), list(ks)

    chunks = []
    pf = _Prefetch(make, [mine[s:s + batch] for s in range(0, len(mine), batch)], dev)
    try:
        for (rgb, meta), ks in pf:
            disp = _disparity(net, rgb)
            _, dec = disp_sample_points(disp, meta[:, :6])
            wrong = (dec != meta[:, 6]).double()
            chunks.append((ks, torch.stack([wrong, dec.double()], 1)))
    finally:
        pf.close()
    table = _collect(chunks, n, world_size)
    wrong = int(round(table[:, 0].sum())) if n else 0
    out = {"WHDR": wrong / n * 100 if n else float("nan"), "wrong": wrong, "total": n}
    if return_decisions:
        out["decisions"] = [chr(int(round(c))) if c else "" for c in table[:, 1]]
    return out
