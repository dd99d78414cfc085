"""Shared by tests/test_png_parallel_cpu.py and tests/test_gpu_png_parallel.py: the streams built for the properties of the
parallel inflate stage (csrc/png_inflate_par.h) beside the files of tests/png_cases.py, and the plans of all of them,
computed once per process."""
import zlib

import numpy as np

import png_cases
from instaorder_amd import png

CHUNKS = (256, 1024)
_cache = {}


W, ROW = 170, 511            # the decoy images: RGB rows of 1 + 510 bytes


def decoy_rows(rows):
    """uint8 [rows, ROW] scanlines, filter type 0, whose pixel bytes are the DEFLATE bytes of the memLevel-1 build (19
    small dynamic blocks): data in which complete dynamic-block headers parse at places that are no block start of the
    stream that carries them"""
    d = png_cases.build(64, 64, "rgb", "mix", seed=3, mem_level=1)[0].deflate_bytes()
    assert len(d) >= rows * (ROW - 1), len(d)
    out = np.zeros((rows, ROW), np.uint8)
    out[:, 1:] = np.frombuffer(d[:rows * (ROW - 1)], np.uint8).reshape(rows, ROW - 1)
    return out


def picture_rows(rows, seed):
    """uint8 [rows, ROW]: a picture's scanlines with a seeded filter type per row (zlib makes dynamic blocks of them)"""
    return png_cases.filtered(png_cases.sample_bytes(png_cases.picture(rows, W, "rgb", seed)), 3,
                              png_cases.row_filters(rows, "mix", seed))


def _image(lines, deflate, name):
    """(PngImage, expected) around scanlines and a DEFLATE stream of them; expected is ``to_host()``, the NumPy rule"""
    raw = lines.tobytes()
    im = png.PngImage(png_cases.png_file(lines.shape[0], W, "rgb", png_cases.zwrap(deflate, raw)), name=name)
    return im, im.to_host()


def stored_decoy():
    """a stored-only stream whose pixels are the bytes of another DEFLATE stream: false candidates, a chain of one"""
    lines = decoy_rows(15)
    return _image(lines, zlib.compress(lines.tobytes(), 0)[2:-4], "stored_decoy")


def decoy_between():
    """two memLevel-1 parts (small dynamic blocks) joined by Z_FULL_FLUSH and one stored block that holds the decoy bytes:
    false candidates that a clean chain of many chunks passes over"""
    lines = np.concatenate([picture_rows(20, 12), decoy_rows(15), picture_rows(20, 14)])
    raw = lines.tobytes()
    a, b = 20 * ROW + 5, 35 * ROW - 7                         # the stored block starts and ends inside a row
    ca, cb = zlib.compressobj(6, zlib.DEFLATED, -15, 1), zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    bits = png_cases.Bits()
    bits.stored(raw[a:b])
    deflate = ca.compress(raw[:a]) + ca.flush(zlib.Z_FULL_FLUSH) + bits.bytes() + cb.compress(raw[b:]) + cb.flush()
    return _image(lines, deflate, "decoy_between")


def property_cases():
    """[(PngImage, expected)]: the three memLevel / Z_HUFFMAN_ONLY builds and the two decoy streams"""
    if "property" not in _cache:
        _cache["property"] = [
            png_cases.build(64, 64, "rgb", "mix", seed=3, mem_level=1, name="memlevel1_small"),
            png_cases.build(96, 96, "rgb", "mix", seed=4, mem_level=2, name="memlevel2_small"),
            png_cases.build(48, 64, "rgb", "mix", seed=5, mem_level=1, strategy=zlib.Z_HUFFMAN_ONLY, name="huffman_only_small"),
            stored_decoy(), decoy_between()]
    return _cache["property"]


def intact_cases():
    """[(PngImage, expected)]: every image of stream_cases(), batch_cases() and property_cases()"""
    if "intact" not in _cache:
        _cache["intact"] = ([c[:2] for c in png_cases.stream_cases()] + list(png_cases.batch_cases()) + property_cases())
    return _cache["intact"]


N_MUTATIONS = 60


def damaged_cases():
    """[(label, PngImage)]: ``png_cases.damaged()`` -- whose three bases have chains of one chunk -- and the memLevel-1
    build with its chain of 18, intact, truncated and mutated the same way: damage behind the first link"""
    if "damaged" not in _cache:
        out = list(png_cases.damaged())
        im = property_cases()[0][0]
        d = im.deflate_bytes()
        out.append((im.name, im))
        out += [("%s cut %d" % (im.name, k), im.with_stream(d[:k], name="%s cut %d" % (im.name, k)))
                for k in png_cases.truncations(len(d))]
        out += [("%s mut %d" % (im.name, m), im.with_stream(png_cases.mutated(d, m), name="%s mut %d" % (im.name, m)))
                for m in range(N_MUTATIONS)]
        _cache["damaged"] = out
    return _cache["damaged"]


def plan(im, chunk_bytes):
    """``im.parallel_plan(chunk_bytes)``, computed once per image object and size"""
    key = (id(im), chunk_bytes)
    if key not in _cache:
        _cache[key] = (im, im.parallel_plan(chunk_bytes))
    return _cache[key][1]


def boundaries(im):
    """(status, {bit behind a block: bytes produced up to it}) of the sequential walk"""
    key = (id(im), "walk")
    if key not in _cache:
        b = []
        status = png.inflate_walk(im.deflate_bytes(), im.inflated_bytes, keep=False, boundaries=b)[0]
        _cache[key] = (im, status, dict(b))
    return _cache[key][1:]
