"""Input pipelines with PNG files decoded on the device (instaorder_amd.png, io_png_decode) against the same files decoded on
the host by Pillow, no network step, one process on one GPU.  The files are generated at start-up from seeds: 1242 x 375
RGB frames (a smooth picture with low-amplitude noise, written by Pillow, whose encoder chooses the row filters) and
16-bit grayscale depth maps of the same size with about 5 % valid points (``synthetic.sparse_gt_u16``) -- the two kinds of
file a KINS / KITTI run reads.

  (a) training pipeline   BatchPrefetcher over SupOcclusionOrderBatches as in tools/jpeg_input_bench.py (run-length masks,
                          a new mask object per item so every item loads and uploads its own frame): ``load_image`` =
                          Pillow (the reference's load) against ``png.PngImage``; batch interval and upload bytes
  (b) dense evaluation    ``dense_eval.eval_dense_depth`` over a KITTI tree of these files with a network that returns a
                          constant map, so what is timed is the input side and the metrics: ``png="host"`` against
                          ``png="device"``; seconds per image
  (c) the stages alone    one ``io_png_decode`` call over 1 and over --images frames / depth maps: inflate (with its
                          Adler-32 launch), unfilter and pack from the library's event timing, per image; and Pillow's
                          decode of the same files on one host thread

The two legs of (a) and of (b) alternate, --repeats times each, in this one run.  The first batch of the legs of (a) and
the rows of (b) must be equal bit for bit; otherwise the exit status is 1.  No threshold on time: a leg that is slower on
the device is reported as it is.

    python tools/png_input_bench.py [--B 64] [--S 256] [--batches 10] [--warmup 3] [--repeats 2] [--images 16] [--out profiles/png_input_bench.json]

With ``--parallel`` the tool compares the two inflate stages instead (``png.set_inflate``): on the same files, for every
``--chunk-bytes`` size, the sequential and the parallel setting alternate, --repeats times each, over the legs one frame
alone, --images frames in one call (and the same for the depth maps), the training pipeline with ``png.PngImage`` and the
dense evaluation's input side with ``png="device"``.  Per size it records chain chunks and fallbacks per file (the info
words), the time of every stage class (search, count with the chain, store, resolve, the predicated sequential kernel
with Adler-32, unfilter, pack) and Pillow's decode time from the same run.  Outputs must be equal bit for bit.

    python tools/png_input_bench.py --parallel [--chunk-bytes 1024 4096 16384] [--out profiles/png_parallel_bench.json]
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rle_input_bench as base  # noqa: E402  (puts the repository root on sys.path)
from instaorder_amd import _lib, dense_eval, png, synthetic  # noqa: E402

H, W = 375, 1242


def frame(seed):
    """a smooth picture with low-amplitude noise, uint8 [H, W, 3]"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    chans = []
    for c in range(3):
        fx, fy, px, py = rng.uniform(0.5, 3.0, 4)
        chans.append(128 + 90 * np.sin(2 * np.pi * (fx * x / W + px)) * np.cos(2 * np.pi * (fy * y / H + py)))
    return np.clip(np.rint(np.stack(chans, 2) + rng.randint(0, 4, (H, W, 3))), 0, 255).astype(np.uint8)


def png_bytes(a):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, "PNG")
    return bio.getvalue()


class FrameReader(base.PerItemRLEReader):
    """the run-length reader with its masks cut or padded to the frame size; ``how`` selects what load_image returns"""

    def __init__(self, reader, files, how):
        base.PerItemRLEReader.__init__(self, reader)
        from PIL import Image
        self._files, self._how, self._Image = files, how, Image
        self.load_seconds, self.load_calls = 0.0, 0
        self._sized = {}

    def get_image_instances(self, idx, *args, **kw):
        from instaorder_amd import rle
        key = int(idx)
        if key not in self._sized:
            out = rle.RLEReader.get_image_instances(self, idx, *args, **kw)
            dense = out[0].to_dense()
            m = np.zeros((dense.shape[0], H, W), np.uint8)
            h, w = min(H, dense.shape[1]), min(W, dense.shape[2])
            m[:, :h, :w] = dense[:, :h, :w]
            self._sized[key] = (rle.RLEMasks.from_dense(m != 0),) + tuple(out[1:])
        out = self._sized[key]
        return (out[0].with_values(out[0].values),) + tuple(out[1:])

    def load_image(self, image_fn):
        t = time.perf_counter()
        if self._how == "pil":
            out = np.array(self._Image.open(io.BytesIO(self._files[image_fn])).convert("RGB"))
        else:
            out = png.PngImage(self._files[image_fn], name=str(image_fn))
        self.load_seconds += time.perf_counter() - t
        self.load_calls += 1
        return out


class ConstantNet(object):
    def _encode_decode(self, rgb):
        return torch.full((rgb.shape[0], rgb.shape[2], rgb.shape[3]), 0.05, device=rgb.device), None


def write_kitti(root, frames, depths):
    lines = []
    for k, (f, d) in enumerate(zip(frames, depths)):
        img_rel = "2011_09_26/2011_09_26_drive_%04d_sync/image_02/data/%010d.png" % (k + 1, k)
        gt_rel = "2011_09_26_drive_%04d_sync/proj_depth/groundtruth/image_02/%010d.png" % (k + 1, k)
        for sub, rel, data in (("rawdata", img_rel, f), ("data_depth_annotated", gt_rel, d)):
            p = os.path.join(root, sub, rel)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "wb") as fh:
                fh.write(data)
        lines.append("%s %s 721.5377" % (img_rel, gt_rel))
    lst = os.path.join(root, "eigen_test.txt")
    with open(lst, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return lst


def stages(ims, label):
    """one io_png_decode call over ``ims`` after a warm one: ms per image of the three classes"""
    L = _lib.lib()
    png.decode(ims, "cuda")
    torch.cuda.synchronize()
    L.io_prof_begin_ex(0)
    t = time.perf_counter()
    png.decode(ims, "cuda")
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    ent = (_lib.ProfEntry * 32)()
    n = L.io_prof_end(ent, 32)
    ms = {e.name.decode(): e.total_ms for e in ent[:n]}
    return dict(files=label, images=len(ims), call_ms=round(1e3 * wall, 3),
                inflate_ms_per_image=round(ms["png_inflate"] / len(ims), 3),
                unfilter_ms_per_image=round(ms["png_unfilter"] / len(ims), 3),
                pack_ms_per_image=round(ms["png_pack"] / len(ims), 4),
                inflate_ms=round(ms["png_inflate"], 3), unfilter_ms=round(ms["png_unfilter"], 3), pack_ms=round(ms["png_pack"], 4))


PAR_CLASSES = ("png_par_search", "png_par_count", "png_par_store", "png_par_resolve", "png_inflate", "png_unfilter", "png_pack")


def stages_setting(ims, mode, chunk_bytes):
    """one decode call over ``ims`` under the setting after a warm one: (call ms, {class: ms}, outputs as bytes, info)"""
    L = _lib.lib()
    keep = png.get_inflate()
    try:
        png.set_inflate(mode, chunk_bytes)
        png.decode(ims, "cuda")
        torch.cuda.synchronize()
        L.io_prof_begin_ex(0)
        t = time.perf_counter()
        got = png.decode(ims, "cuda", info=mode == "parallel")
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        ent = (_lib.ProfEntry * 32)()
        n = L.io_prof_end(ent, 32)
    finally:
        png.set_inflate(keep["mode"], keep["chunk_bytes"])
    ms = {e.name.decode(): round(e.total_ms, 4) for e in ent[:n]}
    tensors, info = got if mode == "parallel" else (got, None)
    return 1e3 * wall, {k: ms.get(k, 0.0) for k in PAR_CLASSES}, [t.cpu().numpy().tobytes() for t in tensors], info


def parallel_main(a):
    """sequential against parallel inflate stage, leg by leg and size by size; the JSON result"""
    import PIL
    from PIL import Image
    rd = synthetic.SyntheticReader(500, n_images=a.images, n_inst=8, max_side=640, min_side=480, empty_every=0)
    rs = np.random.RandomState(77)
    frames = [png_bytes(frame(9000 + i)) for i in range(a.images)]
    depths = [png_bytes(synthetic.sparse_gt_u16(rs, H, W)) for i in range(a.images)]
    files = {rd.get_image_instances(i)[4]: frames[i] for i in range(a.images)}
    fr = [png.PngImage(b, name="frame %d" % i) for i, b in enumerate(frames)]
    dp = [png.PngImage(b, name="depth %d" % i) for i, b in enumerate(depths)]
    pil = {}
    for label, blobs, rgb in (("frame", frames, True), ("depth", depths, False)):
        t = time.perf_counter()
        for b in blobs:
            im = Image.open(io.BytesIO(b))
            np.array(im.convert("RGB") if rgb else im)
        pil[label + "_ms_per_image"] = round(1e3 * (time.perf_counter() - t) / len(blobs), 3)
    ok = True
    sizes = {}
    with tempfile.TemporaryDirectory() as root:
        lst = write_kitti(root, frames, depths)
        for cb in a.chunk_bytes:
            # the stages alone
            alone = []
            for label, ims in (("1 frame", fr[:1]), ("%d frames" % a.images, fr), ("1 depth map", dp[:1]),
                               ("%d depth maps" % a.images, dp)):
                legs = {"sequential": [], "parallel": []}
                ref, info = None, None
                for rep in range(a.repeats):
                    for mode in ("sequential", "parallel"):
                        wall, ms, out, words = stages_setting(ims, mode, cb)
                        legs[mode].append(dict(call_ms=round(wall, 3), classes_ms=ms))
                        ref = out if ref is None else ref
                        ok = ok and out == ref
                        info = words if words is not None else info
                inflate = {m: spread([sum(v for k, v in leg["classes_ms"].items() if k not in ("png_unfilter", "png_pack"))
                                      for leg in legs[m]]) for m in legs}
                alone.append(dict(files=label, images=len(ims), legs=legs, inflate_ms=inflate,
                                  call_ms={m: spread([leg["call_ms"] for leg in legs[m]]) for m in legs},
                                  chain_chunks=[int(w) & 0xFFFF for w in info], fallbacks=int(sum(int(w) >> 16 != 0 for w in info))))
            # the training pipeline and the dense evaluation's input side
            runs = {"sequential": [], "parallel": []}
            secs = {"sequential": [], "parallel": []}
            firsts, rows = [], []
            for rep in range(a.repeats):
                for mode in ("sequential", "parallel"):
                    png.set_inflate(mode, cb)
                    try:
                        reader = FrameReader(rd, files, "png")
                        res, first = base.leg("PngImage, %s inflate at %d, repeat %d" % (mode, cb, rep), reader, a)
                        runs[mode].append(res)
                        firsts.append(first)
                        for warm in (True, False):
                            kr = dense_eval.KITTIEigenReader(lst, root, png="device")
                            torch.cuda.synchronize()
                            t = time.perf_counter()
                            r = dense_eval.eval_dense_depth(ConstantNet(), kr, "midas_pretrained", batch=4, return_rows=True)
                            torch.cuda.synchronize()
                            if not warm:
                                secs[mode].append(1e3 * (time.perf_counter() - t) / a.images)
                        rows.append(r["rows"].tobytes())
                    finally:
                        png.set_inflate("sequential")
            ok = ok and all(np.array_equal(x, y) for f in firsts[1:] for x, y in zip(firsts[0], f)) and len(set(rows)) == 1
            sizes[str(cb)] = dict(stages_alone=alone,
                                  training_batch_ms_median={m: spread([r["batch_ms_median"] for r in runs[m]]) for m in runs},
                                  dense_eval_ms_per_image={m: spread(secs[m]) for m in secs})
        kr = dense_eval.KITTIEigenReader(lst, root, png="host")
        host = []
        for warm in (True, False, False):
            torch.cuda.synchronize()
            t = time.perf_counter()
            dense_eval.eval_dense_depth(ConstantNet(), kr, "midas_pretrained", batch=4, return_rows=True)
            torch.cuda.synchronize()
            if not warm:
                host.append(1e3 * (time.perf_counter() - t) / a.images)
    return dict(tool="tools/png_input_bench.py --parallel", device=torch.cuda.get_device_name(0), csrc_digest=_lib.csrc_digest(),
                B=a.B, S=a.S, batches=a.batches, warmup=a.warmup, repeats=a.repeats, images=a.images,
                files="%d x %d RGB frames (smooth picture, noise 0..3) and 16-bit depth maps (about 5 %% valid), written by "
                      "Pillow %s with its default settings" % (W, H, PIL.__version__),
                frame_file_bytes_mean=round(float(np.mean([len(b) for b in frames])), 1),
                depth_file_bytes_mean=round(float(np.mean([len(b) for b in depths])), 1),
                pillow_decode=pil, dense_eval_host_ms_per_image=spread(host), chunk_bytes=sizes, outputs_equal=bool(ok),
                not_measured="real KITTI files; the pipelines beside a network step; a multi-threaded host decoder"), ok


def spread(v):
    return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3), samples=len(v))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--probe", type=int, default=2)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--out", default="")
    ap.add_argument("--parallel", action="store_true", help="compare the sequential and the parallel inflate stage")
    ap.add_argument("--chunk-bytes", type=int, nargs="+", default=[1024, 4096, 16384])
    a = ap.parse_args(argv)
    assert a.batches >= 1 and a.warmup >= 1 and a.probe >= 1 and a.repeats >= 1 and a.images >= 1
    import PIL
    from PIL import Image
    _lib.require_gpu()
    torch.cuda.set_device(0)
    if a.parallel:
        res, ok = parallel_main(a)
        print(json.dumps({k: v for k, v in res.items() if k != "chunk_bytes"}), flush=True)
        for cb, r in res["chunk_bytes"].items():
            print(json.dumps({"chunk_bytes": int(cb), "training_batch_ms_median": r["training_batch_ms_median"],
                              "dense_eval_ms_per_image": r["dense_eval_ms_per_image"],
                              "stages_alone": [{k: s[k] for k in ("files", "inflate_ms", "call_ms", "fallbacks")}
                                               for s in r["stages_alone"]]}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        if not ok:
            print("FAILED: the legs differ")
        return 0 if ok else 1
    rd = synthetic.SyntheticReader(500, n_images=a.images, n_inst=8, max_side=640, min_side=480, empty_every=0)
    rs = np.random.RandomState(77)
    frames = [png_bytes(frame(9000 + i)) for i in range(a.images)]
    depths = [png_bytes(synthetic.sparse_gt_u16(rs, H, W)) for i in range(a.images)]
    files = {rd.get_image_instances(i)[4]: frames[i] for i in range(a.images)}
    fr = [png.PngImage(b, name="frame %d" % i) for i, b in enumerate(frames)]
    dp = [png.PngImage(b, name="depth %d" % i) for i, b in enumerate(depths)]
    stats = dict(frame=fr[0].stream_stats(), depth=dp[0].stream_stats())
    # (a) the training pipeline
    runs = {"pil": [], "png": []}
    firsts = []
    for rep in range(a.repeats):
        for how, name in (("pil", "PIL in load_image"), ("png", "PngImage (decoded on the device)")):
            reader = FrameReader(rd, files, how)
            res, first = base.leg("%s, repeat %d" % (name, rep), reader, a)
            res["load_image_ms_per_batch"] = round(1e3 * reader.load_seconds / reader.load_calls * a.B, 2)
            runs[how].append(res)
            firsts.append(first)
    same = all(np.array_equal(x, y) for f in firsts[1:] for x, y in zip(firsts[0], f))
    train = dict(legs=runs, batch_ms_median={h: spread([r["batch_ms_median"] for r in runs[h]]) for h in runs},
                 upload_bytes_per_batch={h: runs[h][0]["upload_bytes_per_batch"] for h in runs},
                 png_over_pil_batches_per_s=round(float(np.median([r["batches_per_s"] for r in runs["png"]])
                                                        / np.median([r["batches_per_s"] for r in runs["pil"]])), 3))
    # (b) the dense evaluation's input side
    secs = {"host": [], "device": []}
    rows = {}
    with tempfile.TemporaryDirectory() as root:
        lst = write_kitti(root, frames, depths)
        for rep in range(a.repeats + 1):                         # the first round warms both legs
            for mode in ("host", "device"):
                reader = dense_eval.KITTIEigenReader(lst, root, png=mode)
                torch.cuda.synchronize()
                t = time.perf_counter()
                r = dense_eval.eval_dense_depth(ConstantNet(), reader, "midas_pretrained", batch=4, return_rows=True)
                torch.cuda.synchronize()
                if rep:
                    secs[mode].append(1e3 * (time.perf_counter() - t) / a.images)
                rows[mode] = r["rows"]
    same_rows = rows["host"].tobytes() == rows["device"].tobytes()
    dense = dict(ms_per_image={m: spread(secs[m]) for m in secs}, rows_equal=bool(same_rows), images=a.images, batch=4,
                 device_over_host_images_per_s=round(float(np.median(secs["host"]) / np.median(secs["device"])), 3))
    # (c) the stages alone, and Pillow's decode of the same files
    alone = [stages(fr[:1], "frame"), stages(fr, "frame"), stages(dp[:1], "depth"), stages(dp, "depth")]
    pil = {}
    for label, blobs, rgb in (("frame", frames, True), ("depth", depths, False)):
        t = time.perf_counter()
        for b in blobs:
            im = Image.open(io.BytesIO(b))
            np.array(im.convert("RGB") if rgb else im)
        pil[label + "_ms_per_image"] = round(1e3 * (time.perf_counter() - t) / len(blobs), 3)
    res = dict(tool="tools/png_input_bench.py", device=torch.cuda.get_device_name(0), csrc_digest=_lib.csrc_digest(),
               B=a.B, S=a.S, batches=a.batches, warmup=a.warmup, probe_batches=a.probe, repeats=a.repeats, images=a.images,
               files="%d x %d RGB frames (smooth picture, noise 0..3) and 16-bit depth maps (about 5 %% valid), written by "
                     "Pillow %s with its default settings" % (W, H, PIL.__version__),
               frame_file_bytes_mean=round(float(np.mean([len(b) for b in frames])), 1),
               depth_file_bytes_mean=round(float(np.mean([len(b) for b in depths])), 1),
               frame_pixel_bytes=3 * H * W, depth_pixel_bytes=2 * H * W,
               unfilter="skewed wavefront, bands of %d rows" % _lib.lib().io_png_band_rows(),
               training_pipeline=train, dense_evaluation=dense, stages_alone=alone, pillow_decode=pil,
               first_batch_equal=bool(same), stream_stats=stats,
               not_measured="real KITTI files; the pipelines beside a network step; a multi-threaded host decoder")
    print(json.dumps({k: v for k, v in res.items() if k != "training_pipeline"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not (same and same_rows):
        print("FAILED: the legs differ")
    return 0 if same and same_rows else 1


if __name__ == "__main__":
    sys.exit(main())
