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

With ``--parallel`` the tool compares the two entropy stages of leg 3 instead (``jpeg.set_entropy``): per file set -- the noise
files, and a smooth picture with noise at about 0.6 symbols per pixel -- the legs "JpegImage, sequential entropy" and
"JpegImage, parallel entropy" alternate, ``--repeats`` times each; per leg the entropy class time and the batch interval are
recorded, per set their median and spread, the info-word histogram (rounds, fallbacks) of the set's files, and the entropy
class of both stages with subsequences of 64, 128, 256, 512 and 1024 bytes.  The first batches of a set's legs must be
equal bit for bit.  No threshold: a ratio below 1 is reported as it is.

    python tools/jpeg_input_bench.py --parallel [--repeats 3] [--subseq-bytes 256] [--max-rounds 64] --out profiles/jpeg_parallel_bench.json

With ``--progressive`` the two file sets are encoded with ``progressive=True`` instead and three legs alternate per set,
``--repeats`` times each: "PIL in load_image" -- what becomes of such files without ``jpeg.set_progressive("device")``, so the
baseline --, "JpegImage, progressive stage, scans in file order on one lane" (concurrent 0) and "..., scans of a level side by
side" (concurrent 1), both through io_jpeg_decode_prog_u8.  Per leg the batch interval, the jpeg_prog_entropy class time, the
upload bytes by kind and the cycles per Huffman symbol of that class are recorded, per set their median and spread.  The first
batches of a set's legs must be equal bit for bit.  No threshold: a ratio below 1 is reported as it is.

    python tools/jpeg_input_bench.py --progressive [--repeats 3] --out profiles/jpeg_progressive_bench.json
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


SUBSEQ_SWEEP = (64, 128, 256, 512, 1024)
SMOOTH_SIGMA = 12.0          # noise on the smooth picture: 0.6 Huffman symbols per pixel at quality 90, 4:2:0


def smooth_picture(H, W, seed):
    """a smooth noisy test picture: one slow sine product per channel plus Gaussian noise"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    chans = []
    for c in range(3):
        fx, fy, px, py = rng.uniform(0.5, 3.0, 4)
        chans.append(128 + 90 * np.sin(2 * np.pi * (fx * x / W + px)) * np.cos(2 * np.pi * (fy * y / H + py)))
    img = np.stack(chans, 2) + rng.normal(0.0, SMOOTH_SIGMA, (H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def info_histogram(files, subseq_bytes, max_rounds):
    """the info words of the set's distinct files through one parallel jpeg.decode: rounds -> files, and the fallbacks"""
    keep = jpeg.get_entropy()
    try:
        jpeg.set_entropy("parallel", subseq_bytes, max_rounds)
        ims = [jpeg.JpegImage(b) for b in files.values()]
        _, words = jpeg.decode(ims, "cuda", info=True)
    finally:
        jpeg.set_entropy(keep["mode"], keep["subseq_bytes"], keep["max_rounds"])
    rounds = {}
    for w in words.tolist():
        rounds[str(w & 0xFFFF)] = rounds.get(str(w & 0xFFFF), 0) + 1
    return dict(files=len(ims), rounds=rounds, not_converged=int(sum(1 for w in words.tolist() if w >> 16 == 1)),
                not_clean=int(sum(1 for w in words.tolist() if w >> 16 == 2)),
                subsequences_mean=round(float(np.mean([-(-im.nbytes_entropy // subseq_bytes) for im in ims])), 1))


def entropy_ms(rd, files, a, mode, subseq_bytes, max_rounds):
    """the entropy class per batch from the library's event timing: --repeats probe batches, each timed alone, after a
    warm one; dict(samples, median, min, max) in ms"""
    L = _lib.lib()
    keep = jpeg.get_entropy()
    ms = []
    try:
        jpeg.set_entropy(mode, subseq_bytes, max_rounds)
        ds = base.make(FileReader(rd, files, "jpeg"), a.S)
        idx = base.index_batches(rd.get_image_length(), a.B, 1 + a.repeats)
        ds.batch(idx[0])
        for k in range(a.repeats):
            L.io_prof_begin_ex(0)
            ds.batch(idx[1 + k])
            ent = (_lib.ProfEntry * 32)()
            n = L.io_prof_end(ent, 32)
            ms.append({e.name.decode(): e.total_ms for e in ent[:n]}["jpeg_entropy"])
        ds.renderer.check_status()
    finally:
        jpeg.set_entropy(keep["mode"], keep["subseq_bytes"], keep["max_rounds"])
    return dict(samples=len(ms), median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3))


def parallel_bench(rd, sets, a):
    """sequential against parallel entropy stage (jpeg.set_entropy), per file set: the two legs alternating, --repeats times
    each, then the entropy class over the subsequence sizes.  No threshold; the first batches must be equal."""
    keep = jpeg.get_entropy()
    out, same = [], True
    for set_name, files, sym_per_pixel in sets:
        runs = {"sequential": [], "parallel": []}
        firsts = []
        try:
            for rep in range(a.repeats):
                for mode in ("sequential", "parallel"):
                    jpeg.set_entropy(mode, a.subseq_bytes, a.max_rounds)
                    res, first = run_leg("JpegImage, %s entropy (%s, repeat %d)" % (mode, set_name, rep), rd, files, "jpeg", a)
                    runs[mode].append(dict(batch_ms_median=res["batch_ms_median"], batch_ms_mean=res["batch_ms_mean"],
                                           batch_ms_min_max=res["batch_ms_min_max"],
                                           jpeg_entropy_ms=res["kernels"]["jpeg_entropy"]["ms_per_batch"],
                                           jpeg_idct_ms=res["kernels"]["jpeg_idct"]["ms_per_batch"],
                                           jpeg_colour_ms=res["kernels"]["jpeg_colour"]["ms_per_batch"]))
                    firsts.append(first)
        finally:
            jpeg.set_entropy(keep["mode"], keep["subseq_bytes"], keep["max_rounds"])
        same = same and all(np.array_equal(x, y) for f in firsts[1:] for x, y in zip(firsts[0], f))
        sweep = []
        for size in SUBSEQ_SWEEP:
            seq_ms = entropy_ms(rd, files, a, "sequential", size, a.max_rounds)
            par_ms = entropy_ms(rd, files, a, "parallel", size, a.max_rounds)
            sweep.append(dict(subseq_bytes=size, sequential_entropy_ms=seq_ms, parallel_entropy_ms=par_ms,
                              sequential_over_parallel=round(seq_ms["median"] / par_ms["median"], 3),
                              info=info_histogram(files, size, a.max_rounds)))
            print(json.dumps(sweep[-1]), flush=True)

        def spread(mode, key):
            v = [r[key] for r in runs[mode]]
            return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3))

        summary = {mode: dict(jpeg_entropy_ms=spread(mode, "jpeg_entropy_ms"), batch_ms_median=spread(mode, "batch_ms_median"))
                   for mode in runs}
        out.append(dict(files=set_name, file_bytes_mean=round(float(np.mean([len(b) for b in files.values()])), 1),
                        huffman_symbols_per_pixel=round(sym_per_pixel, 3), subseq_bytes=a.subseq_bytes, max_rounds=a.max_rounds,
                        legs=runs, summary=summary,
                        entropy_sequential_over_parallel=round(summary["sequential"]["jpeg_entropy_ms"]["median"] /
                                                               summary["parallel"]["jpeg_entropy_ms"]["median"], 3),
                        batch_sequential_over_parallel=round(summary["sequential"]["batch_ms_median"]["median"] /
                                                             summary["parallel"]["batch_ms_median"]["median"], 3),
                        info=info_histogram(files, a.subseq_bytes, a.max_rounds), by_subseq_bytes=sweep))
    return out, same


def progressive_bench(rd, sets, a, clock_mhz):
    """Pillow in load_image against the progressive stage with concurrent 0 and 1, per file set: the three legs alternating,
    --repeats times each.  No threshold; the first batches must be equal."""
    legs_of = (("PIL in load_image", "pil", None), ("JpegImage, progressive stage, scans in file order on one lane", "jpeg", 0),
               ("JpegImage, progressive stage, scans of a level side by side", "jpeg", 1))
    out, same = [], True
    for set_name, files, sym_per_pixel, pixels in sets:
        runs = {name: [] for name, _, _ in legs_of}
        firsts = []
        try:
            for rep in range(a.repeats):
                for name, how, concurrent in legs_of:
                    jpeg.set_progressive("host" if concurrent is None else "device", concurrent or 0)
                    res, first = run_leg("%s (%s, repeat %d)" % (name, set_name, rep), rd, files, how, a)
                    ms = res["kernels"].get("jpeg_prog_entropy", {}).get("ms_per_batch")
                    runs[name].append(dict(batch_ms_median=res["batch_ms_median"], batch_ms_mean=res["batch_ms_mean"],
                                           batch_ms_min_max=res["batch_ms_min_max"], jpeg_prog_entropy_ms=ms,
                                           load_image_ms_per_batch=res["load_image_ms_per_batch"],
                                           upload_bytes_per_batch=res["upload_bytes_per_batch"],
                                           # one block per image, all at once: the class lasts as long as an image's scans do
                                           cycles_per_symbol=None if ms is None else round(
                                               ms * 1e-3 * clock_mhz * 1e6 / (sym_per_pixel * pixels), 1)))
                    firsts.append(first)
        finally:
            jpeg.set_progressive("host")
        same = same and all(np.array_equal(x, y) for f in firsts[1:] for x, y in zip(firsts[0], f))

        def spread(name, key):
            v = [r[key] for r in runs[name] if r[key] is not None]
            return dict(median=round(float(np.median(v)), 3), min=round(min(v), 3), max=round(max(v), 3)) if v else None

        summary = {name: dict(batch_ms_median=spread(name, "batch_ms_median"), jpeg_prog_entropy_ms=spread(name, "jpeg_prog_entropy_ms"),
                              cycles_per_symbol=spread(name, "cycles_per_symbol")) for name in runs}
        pil = summary[legs_of[0][0]]["batch_ms_median"]["median"]
        out.append(dict(files=set_name, file_bytes_mean=round(float(np.mean([len(b) for b in files.values()])), 1),
                        pixel_bytes_mean=round(3 * pixels, 1), huffman_symbols_per_pixel=round(sym_per_pixel, 3), legs=runs,
                        summary=summary,
                        pil_over_one_lane_batch=round(pil / summary[legs_of[1][0]]["batch_ms_median"]["median"], 3),
                        pil_over_side_by_side_batch=round(pil / summary[legs_of[2][0]]["batch_ms_median"]["median"], 3),
                        one_lane_over_side_by_side_entropy=round(summary[legs_of[1][0]]["jpeg_prog_entropy_ms"]["median"] /
                                                                 summary[legs_of[2][0]]["jpeg_prog_entropy_ms"]["median"], 3)))
    return out, same


def symbols_per_pixel(blobs, progressive=None):
    ims = [jpeg.JpegImage(b, progressive=progressive) for b in blobs]
    stats = [{} for _ in ims]
    for im, st in zip(ims, stats):
        im.coefficients(st)
    return sum(st["symbols"] for st in stats) / float(sum(im.H * im.W for im in ims))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--probe", type=int, default=3)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--out", default="")
    ap.add_argument("--parallel", action="store_true",
                    help="compare the sequential and the parallel entropy stage instead of the three legs (profiles/jpeg_parallel_bench.json)")
    ap.add_argument("--progressive", action="store_true",
                    help="Pillow against the progressive stage on progressive files instead (profiles/jpeg_progressive_bench.json)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--subseq-bytes", type=int, default=256)
    ap.add_argument("--max-rounds", type=int, default=64)
    a = ap.parse_args(argv)
    assert a.batches >= 1 and a.warmup >= 1 and a.probe >= 1 and a.repeats >= 1
    from PIL import Image, features
    _lib.require_gpu()
    torch.cuda.set_device(0)
    rd = synthetic.SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0)
    files = {}
    for i, sc in enumerate(rd.scenes):
        bio = io.BytesIO()
        Image.fromarray(sc["image"]).save(bio, "JPEG", quality=90, subsampling=2)
        files[rd.get_image_instances(i)[4]] = bio.getvalue()
    if a.progressive:
        sets = []
        for set_name, picture in (("uniform noise", lambda i, sc: sc["image"]),
                                  ("smooth picture with noise (sigma %g)" % SMOOTH_SIGMA,
                                   lambda i, sc: smooth_picture(sc["image"].shape[0], sc["image"].shape[1], 9000 + i))):
            prog = {}
            for i, sc in enumerate(rd.scenes):
                bio = io.BytesIO()
                Image.fromarray(picture(i, sc)).save(bio, "JPEG", quality=90, subsampling=2, progressive=True)
                prog[rd.get_image_instances(i)[4]] = bio.getvalue()
            sets.append((set_name, prog, symbols_per_pixel(list(prog.values())[:1], progressive=True),
                         float(np.mean([sc["image"].shape[0] * sc["image"].shape[1] for sc in rd.scenes]))))
        props = torch.cuda.get_device_properties(0)
        clock_mhz = props.clock_rate / 1e3 if hasattr(props, "clock_rate") else 2400.0
        results, same = progressive_bench(rd, sets, a, clock_mhz)
        res = dict(tool="tools/jpeg_input_bench.py --progressive", device=torch.cuda.get_device_name(0),
                   csrc_digest=_lib.csrc_digest(), B=a.B, S=a.S, batches=a.batches, warmup=a.warmup, probe_batches=a.probe,
                   repeats=a.repeats, libjpeg=str(features.version("jpg")), shader_clock_mhz=clock_mhz,
                   reader="SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0), run-length "
                          "masks, a new mask object (so an image load and upload) per item; both file sets progressive 4:2:0, "
                          "quality 90, encoded once with Pillow (its ten-scan script); every image of a batch is progressive",
                   first_batch_equal=bool(same), sets=results,
                   samples="one timed leg of --batches batches per repeat, the three legs alternating; summary = median / min / "
                           "max over the repeats; the symbol count is that of one file of the set, scaled by the pixels",
                   not_measured="real COCO files; batches that mix progressive and baseline files; the pipeline beside a network "
                                "step; a multi-threaded host decoder; the shader clock during the run (cycles assume the value given)")
        print(json.dumps({k: v for k, v in res.items() if k != "sets"}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        if not same:
            print("FAILED: the first batch of the legs differs")
        return 0 if same else 1
    if a.parallel:
        smooth = {}
        for i, sc in enumerate(rd.scenes):
            bio = io.BytesIO()
            Image.fromarray(smooth_picture(sc["image"].shape[0], sc["image"].shape[1], 9000 + i)).save(bio, "JPEG", quality=90,
                                                                                                       subsampling=2)
            smooth[rd.get_image_instances(i)[4]] = bio.getvalue()
        sets = [("uniform noise", files, symbols_per_pixel(list(files.values())[:2])),
                ("smooth picture with noise (sigma %g)" % SMOOTH_SIGMA, smooth, symbols_per_pixel(list(smooth.values())[:2]))]
        results, same = parallel_bench(rd, sets, a)
        res = dict(tool="tools/jpeg_input_bench.py --parallel", device=torch.cuda.get_device_name(0),
                   csrc_digest=_lib.csrc_digest(), B=a.B, S=a.S, batches=a.batches, warmup=a.warmup, probe_batches=a.probe,
                   repeats=a.repeats, libjpeg=str(features.version("jpg")),
                   reader="SyntheticReader(500, n_images=32, n_inst=8, max_side=640, min_side=480, empty_every=0), run-length "
                          "masks, a new mask object (so an image load and upload) per item; both file sets baseline 4:2:0, "
                          "quality 90, encoded once with Pillow",
                   first_batch_equal=bool(same), sets=results,
                   samples="legs: one timed leg of --batches batches per repeat, summary = median / min / max over the repeats; "
                           "by_subseq_bytes: --repeats probe batches per size and stage, each timed alone (samples, median, min, "
                           "max); info: the rounds and fallbacks follow from the files and the setting alone (the scheme is "
                           "deterministic), so they are recorded once per set and size, not per leg",
                   not_measured="real COCO files; the pipeline beside a network step; files with restart intervals; the "
                                "shader clock during the run")
        print(json.dumps({k: v for k, v in res.items() if k != "sets"}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        if not same:
            print("FAILED: the first batch of the legs differs")
        return 0 if same else 1
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
                            "network step; a multi-threaded host decoder; the shader clock during the run (cycles assume the value "
                            "given).  Several lanes on one image: --parallel")
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
