"""Input pipeline with JPEG images decoded on the device (instaorder_amd.jpeg) against the same files decoded on the host, no
network step: the legs of tools/rle_input_bench.py (BatchPrefetcher over SupOcclusionOrderBatches, the reader of ``bench.py
--host-inputs u8``, B = 256 pairs at S = 256, one process on one GPU).  The reader's 32 images are encoded once at start-up
with Pillow as baseline 4:2:0 files of quality 90 -- they are uniform noise, about the worst a JPEG coder meets: 1.3
Huffman symbols per pixel and a file a third of the pixels, where a photograph has 0.3 to 0.6 and a fifth to an eighth --
and every leg sees the pixels libjpeg makes of those files.  Masks are run-length coded and a new mask object is handed
out per item, so every item loads and uploads its own image, as a training set with one pair per image does.

  1. arrays              the files decoded before the timing starts: the path as it was, the host decode hidden
  2. PIL in load_image   ``np.array(Image.open(f).convert('RGB'))`` per item, the reference's own load: the baseline
  3. JpegImage           the bytes parsed per item (``jpeg.JpegImage``), decoded by io_jpeg_decode_u8

Per leg: batches/s (median, mean, min-max interval), the bytes one batch uploads by kind, the host time inside load_image
per batch, and the kernel times per batch from the library's event timing, the three decode stages among them.  For leg 3
also the entropy stage's time and cycles per Huffman symbol with 64, 16, 4 and 1 images per wave64.  The first probe batch
of all legs must be equal bit for bit; otherwise the exit status is 1.  No threshold on time or bytes.

    python tools/jpeg_input_bench.py [--batches 20] [--warmup 5] [--B 256] [--S 256] [--out profiles/jpeg_input_bench.json]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rle_input_bench as base  # noqa: E402  (puts the repository root on sys.path)
from instaorder_amd import _lib, jpeg, rle, synthetic  # noqa: E402


class FileReader(base.PerItemRLEReader):
    """the run-length reader over ``files`` = {image_fn: JPEG bytes}; ``how`` selects what load_image returns"""

    def __init__(self, reader, files, how):
        base.PerItemRLEReader.__init__(self, reader)
        from PIL import Image
        self._files, self._how, self._Image = files, how, Image
        self._arrays = {fn: self._pil(b) for fn, b in files.items()} if how == "arrays" else None
        self.load_seconds, self.load_calls = 0.0, 0

    def _pil(self, b):
        return np.array(self._Image.open(io.BytesIO(b)).convert("RGB"))

    def load_image(self, image_fn):
        t = time.perf_counter()
        if self._how == "arrays":
            out = self._arrays[image_fn]
        elif self._how == "pil":
            out = self._pil(self._files[image_fn])
        else:
            out = jpeg.JpegImage(self._files[image_fn], name=str(image_fn))
        self.load_seconds += time.perf_counter() - t
        self.load_calls += 1
        return out


def run_leg(name, rd, files, how, a):
    reader = FileReader(rd, files, how)
    res, first = base.leg(name, reader, a)
    res["load_image_ms_per_batch"] = round(1e3 * reader.load_seconds / reader.load_calls * a.B, 2)
    return res, first


def entropy_sweep(rd, files, a, symbols_per_batch, clock_mhz):
    """the entropy stage with fewer images per wave: one probe batch each"""
    L = _lib.lib()
    keep = L.io_jpeg_get_images_per_wave()
    rows = []
    try:
        for per_wave in (64, 16, 4, 1):
            L.io_jpeg_set_images_per_wave(per_wave)
            ds = base.make(FileReader(rd, files, "jpeg"), a.S)
            idx = base.index_batches(rd.get_image_length(), a.B, 2)
            ds.batch(idx[0])                                     # warm
            L.io_prof_begin_ex(0)
            ds.batch(idx[1])
            ent = (_lib.ProfEntry * 32)()
            n = L.io_prof_end(ent, 32)
            ms = {e.name.decode(): e.total_ms for e in ent[:n]}["jpeg_entropy"]
            # every lane decodes its image alone: the stage lasts as long as its slowest image
            rows.append(dict(images_per_wave=per_wave, entropy_ms=round(ms, 3),
                             cycles_per_symbol_per_lane=round(ms * 1e-3 * clock_mhz * 1e6 / (symbols_per_batch / a.B), 1)))
            ds.renderer.check_status()
    finally:
        L.io_jpeg_set_images_per_wave(keep)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--probe", type=int, default=3)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    assert a.batches >= 1 and a.warmup >= 1 and a.probe >= 1
    from PIL import Image, features
    _lib.require_gpu()
    torch.cuda.set_device(0)
    rd = synthetic.SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0)
    files = {}
    for i, sc in enumerate(rd.scenes):
        bio = io.BytesIO()
        Image.fromarray(sc["image"]).save(bio, "JPEG", quality=90, subsampling=2)
        files[rd.get_image_instances(i)[4]] = bio.getvalue()
    pixels = float(np.mean([sc["image"].shape[0] * sc["image"].shape[1] for sc in rd.scenes]))
    some = list(files.values())[:2]                              # the symbol count of two files, scaled by the pixels
    stats = [{} for _ in some]
    ims = [jpeg.JpegImage(b) for b in some]
    for im, st in zip(ims, stats):
        im.coefficients(st)
    sym_per_pixel = sum(st["symbols"] for st in stats) / float(sum(im.H * im.W for im in ims))
    legs, firsts = [], []
    for name, how in (("arrays (decoded before the timing starts)", "arrays"), ("PIL in load_image", "pil"),
                      ("JpegImage (decoded on the device)", "jpeg")):
        res, first = run_leg(name, rd, files, how, a)
        legs.append(res)
        firsts.append(first)
    same = all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(*firsts))
    clock_mhz = torch.cuda.get_device_properties(0).clock_rate / 1e3 if hasattr(torch.cuda.get_device_properties(0),
                                                                               "clock_rate") else 2400.0
    sweep = entropy_sweep(rd, files, a, sym_per_pixel * pixels * a.B, clock_mhz)
    res = dict(tool="tools/jpeg_input_bench.py", device=torch.cuda.get_device_name(0), csrc_digest=_lib.csrc_digest(),
               B=a.B, S=a.S, batches=a.batches, warmup=a.warmup, probe_batches=a.probe,
               reader="SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0), run-length "
                      "masks, a new mask object (so an image load and upload) per item",
               files="the reader's uniform-noise images encoded once with Pillow: baseline, 4:2:0, quality 90",
               libjpeg=str(features.version("jpg")), file_bytes_mean=round(float(np.mean([len(b) for b in files.values()])), 1),
               pixel_bytes_mean=round(3 * pixels, 1), huffman_symbols_per_pixel=round(sym_per_pixel, 3),
               shader_clock_mhz=clock_mhz, legs=legs, first_batch_equal=bool(same), entropy_stage_by_images_per_wave=sweep,
               jpeg_over_pil_batches_per_s=round(legs[2]["batches_per_s"] / legs[1]["batches_per_s"], 3),
               jpeg_over_arrays_batches_per_s=round(legs[2]["batches_per_s"] / legs[0]["batches_per_s"], 3),
               not_measured="real COCO files (photographs have a third of these symbols per pixel); the pipeline beside a "
                            "network step; a multi-threaded host decoder; several lanes working on one image; the shader clock during the run (cycles assume the value given); restart "
                            "intervals decoded in parallel")
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not same:
        print("FAILED: the first batch of the legs differs")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
