"""The parallel inflate stage on the host: ``PngImage.parallel_plan`` (the rule of csrc/png_inflate_par.h in Python) against
the sequential walk on every intact and damaged stream at two chunk sizes, the stream properties the inputs were built
for, the settings and bindings, and the header itself compiled for the CPU with the waves simulated in order under the
sanitizers (tests/png_parallel_host.cpp).  All comparisons are exact; nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import png_cases
import png_parallel_cases as cases
from helpers import ROOT
from instaorder_amd import _lib, png

CHUNKS = cases.CHUNKS


def by_name(name):
    return next(im for im, _ in cases.intact_cases() if im.name == name)


def false_candidates(im, plan):
    """candidates that are no block start of the stream"""
    bnd = cases.boundaries(im)[1]
    return sum(1 for c, s in enumerate(plan["starts"]) if c > 0 and s >= 0 and s not in bnd)


def test_plan_against_the_sequential_walk():
    parallel = 0
    for im, _ in cases.intact_cases():
        status, bnd = cases.boundaries(im)
        raw_status, raw = im.inflate_status()
        assert status == raw_status == 0, im.name
        for cb in CHUNKS:
            p = cases.plan(im, cb)
            what = (im.name, cb)
            assert p["chunks"] == -(-len(im.deflate_bytes()) // cb) == len(p["starts"]) == len(p["records"]), what
            assert p["starts"][0] == 0 and p["chain"][0] == 0 and p["offsets"][0] == 0, what
            for c, s in enumerate(p["starts"]):
                assert s == -1 or 8 * c * cb <= s < min(8 * (c + 1) * cb, 8 * len(im.deflate_bytes())), what
                assert (s >= 0) == (p["records"][c] is not None), what
            assert p["clean"] and (p["info"] >> 16 == 0) == p["parallel"] == (len(p["chain"]) >= 2), what
            assert p["info"] & 0xFFFF == len(p["chain"]), what
            for c, o in zip(p["chain"][1:], p["offsets"][1:]):           # every link is a block boundary of the walk ...
                assert bnd.get(p["starts"][c]) == o, what               # ... and its offset the bytes produced there
            assert sum(p["records"][c]["n"] for c in p["chain"]) == im.inflated_bytes, what
            last = p["records"][p["chain"][-1]]
            assert last["exit"] == png.EXIT_FINAL and last["exit_bit"] == max(bnd), what
            for c, o, sym in zip(p["chain"], p["offsets"], p["symbols"]):
                assert sym.dtype == np.uint16 and sym.size == p["records"][c]["n"], what
                marks = sym[sym >= 0x8000].astype(np.int64) & 0x7FFF
                assert marks.size == 0 or marks.max() < min(o, 32768), what        # a marker never reaches before byte 0
            if p["parallel"]:
                assert p["resolved"] == raw, what
                parallel += 1
            else:
                assert p["resolved"] is None and p["info"] == png.INFO_CHAIN_OF_ONE | 1, what
    assert parallel >= 16


def test_inputs_have_the_properties_they_were_built_for():
    p = cases.plan(by_name("memlevel1_small"), 256)                      # a long chain
    assert len(p["chain"]) >= 8 and p["parallel"], len(p["chain"])
    assert len(cases.plan(by_name("memlevel1_small"), 1024)["chain"]) >= 4
    p = cases.plan(by_name("several_dynamic"), 256)                      # a chunk whose symbols wrap the rings twice
    assert p["parallel"] and max(p["records"][c]["n"] for c in p["chain"]) > 65536
    for name in ("memlevel1_small", "memlevel2_small", "decoy_between"):  # markers, copied markers, a far reach
        for cb in CHUNKS:
            st = cases.plan(by_name(name), cb)["stats"]
            assert st["markers"] > 0 and st["markers_copied"] > 0 and st["reach_chunks"] > 1, (name, cb, st)
            assert st["fixed"] >= 1 and st["stored"] >= 1 and st["dynamic"] >= 2, (name, cb, st)   # inside chain chunks
    assert cases.plan(by_name("ring_wraps"), 1024)["stats"]["max_reach"] > 24576
    for cb in CHUNKS:
        im = by_name("decoy_between")                                    # false candidates beside a clean chain
        p = cases.plan(im, cb)
        assert p["parallel"] and len(p["chain"]) >= 2 and false_candidates(im, p) >= 1, (cb, false_candidates(im, p))
        ends = {(r["exit"], r["status"]) for c, r in enumerate(p["records"]) if r is not None and c not in p["chain"]}
        assert len(ends) >= 4, ends                                      # the wasted decodes end in many ways
        im = by_name("stored_decoy")                                     # ... and beside a chain of one
        p = cases.plan(im, cb)
        assert p["clean"] and p["info"] == png.INFO_CHAIN_OF_ONE | 1 and false_candidates(im, p) >= 1
    # no false candidate at any bit of the ordinary streams
    for name in ("several_dynamic", "ring_wraps", "memlevel1_small", "memlevel2_small", "huffman_only_small"):
        im = by_name(name)
        bnd = cases.boundaries(im)[1]
        assert all(b in bnd or b == 0 for b in png.dynamic_header_bits(im.deflate_bytes())), name


def test_damaged_streams_fall_back_exactly_when_they_must():
    """The plan hands a stream to the sequential kernel (bit 16 or 17) exactly when the inflate loop gives it a status word
    or its chain has one chunk.  The Adler-32 (status 8 of ``inflate_status``) is a later stage on both paths: a stream that
    inflates to the right count with other bytes is clean."""
    seen = set()
    both = 0
    for label, im in cases.damaged_cases():
        walk = png.inflate_walk(im.deflate_bytes(), im.inflated_bytes, keep=False)[0]
        full = im.inflate_status()[0]
        assert full == walk or (walk == 0 and full == 8), label
        for cb in CHUNKS:
            p = cases.plan(im, cb)
            fallback = p["info"] >> 16 != 0
            assert fallback == (walk != 0 or len(p["chain"]) == 1 or p["chunks"] == 0), (label, cb, walk, hex(p["info"]))
            assert p["clean"] == (walk == 0 and p["chunks"] > 0), (label, cb, walk)
            assert not (walk != 0 and p["clean"]) and bool(p["info"] & png.INFO_NOT_CLEAN) == (not p["clean"]), (label, cb)
            seen.add((walk, fallback))
            both += walk != 0 and len(p["chain"]) >= 2
    assert {s for s, _ in seen} == set(range(8)) and (0, False) in seen, sorted(seen)
    assert both >= 20                                                    # damage behind the first link is there


def test_settings():
    assert png.get_inflate() == dict(mode="sequential", chunk_bytes=png.DEFAULT_CHUNK_BYTES)
    try:
        png.set_inflate("parallel", 4096)
        assert png.get_inflate() == dict(mode="parallel", chunk_bytes=4096)
        assert png.get_inflate("sequential") == dict(mode="sequential", chunk_bytes=4096)
        got = png.get_inflate()
        got["mode"] = "x"
        assert png.get_inflate()["mode"] == "parallel"                   # a copy
        for bad in (0, 255, 300, 128, (1 << 20) + 256, -256, 256.0, "256", None, True):
            with pytest.raises(ValueError, match="chunk_bytes"):
                png.set_inflate("parallel", bad)
        for bad in ("fast", "", None, 1):
            with pytest.raises(ValueError, match="mode"):
                png.set_inflate(bad)
        with pytest.raises(ValueError, match="inflate"):
            png.get_inflate("fast")
        assert png.get_inflate() == dict(mode="parallel", chunk_bytes=4096)      # a refused call changes nothing
        png.set_inflate("parallel", 1 << 20)
        png.set_inflate("sequential")
        assert png.get_inflate() == dict(mode="sequential", chunk_bytes=png.DEFAULT_CHUNK_BYTES)
    finally:
        png.set_inflate("sequential")
    assert png.get_inflate()["mode"] == "sequential"
    # the environment variable is read at import: a fresh interpreter per value (no GPU is touched)
    code = "from instaorder_amd import png; print(png.get_inflate()['mode'], png.get_inflate()['chunk_bytes'])"
    for value, want in (("parallel", "parallel %d" % png.DEFAULT_CHUNK_BYTES), ("", "sequential %d" % png.DEFAULT_CHUNK_BYTES),
                        ("gpu", None)):
        env = dict(os.environ, IO_PNG_INFLATE=value)
        run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        if want is None:
            assert run.returncode != 0 and "png.set_inflate: mode 'gpu'" in run.stderr, run.stderr[-2000:]
        else:
            assert run.returncode == 0 and run.stdout.strip() == want, (value, run.stdout, run.stderr[-2000:])
    with pytest.raises(ValueError, match="chunk_bytes"):
        png_cases.build(7, 5)[0].parallel_plan(100)


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    for name, nargs in (("io_png_decode_par", 13), ("io_png_par_workspace_bytes", 3)):
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name + " is not declared in include/instaorder_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(_lib.lib(), name), name
    assert _lib.SIGNATURES["io_png_decode_par"][1][:10] == _lib.SIGNATURES["io_png_decode"][1][:10]
    mk = open(os.path.join(ROOT, "instaorder_amd", "csrc", "Makefile")).read()
    assert "png_inflate_par.h" in mk
    par = open(os.path.join(ROOT, "instaorder_amd", "csrc", "png_inflate_par.h")).read()
    for name, value in (("PNG_PAR_MIN_CHUNK", png.PAR_MIN_CHUNK), ("PNG_PAR_MAX_CHUNKS", png.PAR_MAX_CHUNKS),
                        ("PNG_INFO_NOT_CLEAN", png.INFO_NOT_CLEAN), ("PNG_INFO_CHAIN_OF_ONE", png.INFO_CHAIN_OF_ONE)):
        m = re.search(r"#define %s \(?(\d+)(?: << (\d+))?\)?" % name, par)
        assert m and int(m.group(1)) << int(m.group(2) or 0) == value, name
    assert png.PAR_MAX_CHUNK == 1 << 20 and "#define PNG_PAR_MAX_CHUNK (1 << 20)" in par
    for name in ("EXIT_NONE", "EXIT_FINAL", "EXIT_LINK", "EXIT_STATUS"):
        assert re.search(r"PNG_%s = %d\b" % (name, getattr(png, name)), par), name


def test_workspace_bytes_follow_the_formula_of_the_header():
    ims = [im for im, _ in cases.property_cases()] + [c[0] for c in png_cases.batch_cases()[:5]]
    pool, desc = png.descriptors(ims, [0] * len(ims))
    n = len(ims)
    r16 = lambda x: (x + 15) // 16 * 16
    units = sum((im.inflated_bytes + 15) // 16 for im in ims)
    sequential = png.workspace_bytes(desc, "sequential")
    assert sequential == r16(8 * (n + 1)) + 16 * units
    for cb in (256, 1024, 1 << 20):
        chunks = sum(-(-len(im.deflate_bytes()) // cb) for im in ims)
        want = sequential + 32 * units + r16(8 * (n + 1)) + r16(8 * n) + 48 * chunks
        assert png.workspace_bytes(desc, dict(mode="parallel", chunk_bytes=cb)) == want, cb
        assert int(_lib.lib().io_png_par_workspace_bytes(C.cast(desc, C.c_void_p), n, cb)) == want
    for bad in (0, 128, 300, (1 << 20) + 256, -256):
        assert int(_lib.lib().io_png_par_workspace_bytes(C.cast(desc, C.c_void_p), n, bad)) == 0
        assert "chunk_bytes" in _lib.last_error()
    big = (_lib.PngDesc * 1)()
    C.memmove(big, C.byref(desc[0]), 48)
    big[0].data_bytes = 256 * 65535 + 1                                  # 65536 chunks of 256 bytes
    assert int(_lib.lib().io_png_par_workspace_bytes(C.cast(big, C.c_void_p), 1, 256)) == 0 and "chunks" in _lib.last_error()
    assert int(_lib.lib().io_png_par_workspace_bytes(C.cast(big, C.c_void_p), 1, 512)) > 0
    big[0].H = 0
    with pytest.raises(RuntimeError, match="io_png_par_workspace_bytes refused"):
        png.workspace_bytes(big, dict(mode="parallel", chunk_bytes=512))
    try:                                                                 # the module-wide setting decides by default
        png.set_inflate("parallel", 256)
        assert png.workspace_bytes(desc) > sequential
    finally:
        png.set_inflate("sequential")
    assert png.workspace_bytes(desc) == sequential


def test_parallel_inflate_under_the_sanitizers(tmp_path):
    """csrc/png_inflate_par.h compiled for the CPU with AddressSanitizer and UBSan, the waves simulated in order: all of
    ``damaged()`` and the intact streams at both chunk sizes, every workspace region in a heap block of its exact size.  The
    program compares each result with the sequential ``png_inflate`` of the same header, byte for byte and status for
    status; here the status is also the word of ``inflate_walk`` and the info word that of ``parallel_plan``."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "png_parallel_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "instaorder_amd", "csrc"),
                            os.path.join(ROOT, "tests", "png_parallel_host.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    ims = [im for _, im in cases.damaged_cases()] + [im for im, _ in cases.intact_cases()]
    rec = str(tmp_path / "streams.bin")
    with open(rec, "wb") as f:
        f.write(png_cases.host_records(ims))
    run = subprocess.run([exe, rec] + [str(cb) for cb in CHUNKS], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    rows = [[int(v) for v in ln.split()] for ln in run.stdout.splitlines()]
    assert len(rows) == len(ims) * len(CHUNKS)
    stored = 0
    for k, (idx, cb, info, status, par) in enumerate(rows):
        im = ims[k // len(CHUNKS)]
        assert idx == k // len(CHUNKS) and cb == CHUNKS[k % len(CHUNKS)]
        assert status == png.inflate_walk(im.deflate_bytes(), im.inflated_bytes, keep=False)[0], (im.name, cb, status)
        assert info == cases.plan(im, cb)["info"], (im.name, cb, hex(info))
        assert par == (info >> 16 == 0)
        stored += par
    assert stored >= 40
