"""The parallel entropy stage of the JPEG decoder on the host: the declarations, the refusals that need no GPU,
``JpegImage.parallel_plan`` (csrc/jpeg_sync.h in Python, the contract of the info word) against ``coefficients()`` on every
fixture file, and the header itself built for the CPU and run under the sanitizers on intact, truncated and mutated
streams (tests/jpeg_parallel_host.cpp).  All comparisons are exact; nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases
from helpers import ROOT
from instaorder_amd import _lib, jpeg

NAMES, CASES, _ = jpeg_cases.load()
SIZES = (16, 24, 256)


def subsequences(im, size):
    return max(1, -(-im.nbytes_entropy // size))


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    for name, nargs in (("io_jpeg_decode_par_u8", 17), ("io_jpeg_par_workspace_bytes", 3), ("io_jpeg_decode_u8", 14),
                        ("io_jpeg_workspace_bytes", 2)):
        decl = re.search(r"\b(?:int|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name + " is not declared in include/instaorder_hip.h"
        assert len(decl.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
    # the 13 arguments in front are those of io_jpeg_decode_u8
    assert _lib.SIGNATURES["io_jpeg_decode_par_u8"][1][:13] == _lib.SIGNATURES["io_jpeg_decode_u8"][1][:13]
    lib = _lib.lib()
    assert hasattr(lib, "io_jpeg_decode_par_u8") and hasattr(lib, "io_jpeg_par_workspace_bytes")
    assert lib.io_abi_version() == 1
    mk = open(os.path.join(ROOT, "instaorder_amd", "csrc", "Makefile")).read()
    assert "jpeg_sync.h" in mk
    sync = open(os.path.join(ROOT, "instaorder_amd", "csrc", "jpeg_sync.h")).read()
    assert '#include "jpeg_entropy.h"' in sync
    assert int(sync.split("#define JPEG_INFO_NOT_CONVERGED (1 <<")[1].split(")")[0]) == 16
    assert int(sync.split("#define JPEG_INFO_NOT_CLEAN (1 <<")[1].split(")")[0]) == 17


def test_workspace_refusals_and_size():
    ims = [jpeg_cases.image(n) for n in ("9x17_420_q85", "21x35_422_q85", "33x47_444_q85", "40x24_gray_q85", "1x1_420_q85")]
    pool, tables, desc = jpeg.descriptors(ims, [0] * len(ims))
    seq = jpeg.workspace_bytes(desc, "sequential")
    assert seq == jpeg.workspace_bytes(desc)                     # the module default is the sequential stage
    assert jpeg.get_entropy() == dict(mode="sequential", subseq_bytes=256, max_rounds=64)
    L = _lib.lib()
    for size in SIZES + (4096,):
        subs = sum(subsequences(im, size) for im in ims)
        head = ((len(ims) + 1) * 8 + 15 & ~15) + (len(ims) * 4 + 15 & ~15)
        assert int(L.io_jpeg_par_workspace_bytes(C.cast(desc, C.c_void_p), len(desc), size)) == (seq + 15 & ~15) + head + 64 * subs
    for size in (8, 20, 8192, 0, -16):
        assert int(L.io_jpeg_par_workspace_bytes(C.cast(desc, C.c_void_p), len(desc), size)) == 0, size
        assert "subseq_bytes" in _lib.last_error()
    for field, value in (("hs", 3), ("n_comp", 2), ("H", 0), ("W", 70000), ("restart_interval", -1), ("table_set", -1)):
        bad = (_lib.JpegDesc * 1)()
        C.memmove(bad, C.byref(desc[0]), 64)
        setattr(bad[0], field, value)
        assert int(L.io_jpeg_par_workspace_bytes(C.cast(bad, C.c_void_p), 1, 256)) == 0, field
        with pytest.raises(RuntimeError, match="refused"):
            jpeg.workspace_bytes(bad, "parallel")
    assert int(L.io_jpeg_par_workspace_bytes(None, 1, 256)) == 0 and int(L.io_jpeg_par_workspace_bytes(C.cast(desc, C.c_void_p), 0, 256)) == 0


def test_set_entropy_checks_its_arguments():
    keep = jpeg.get_entropy()
    try:
        jpeg.set_entropy("parallel", subseq_bytes=64, max_rounds=9)
        assert jpeg.get_entropy() == dict(mode="parallel", subseq_bytes=64, max_rounds=9)
        assert jpeg.get_entropy("sequential")["mode"] == "sequential"
        for args in (("both",), ("parallel", 20), ("parallel", 8), ("parallel", 8192), ("parallel", 256, 0), ("parallel", 256, 65536)):
            with pytest.raises(ValueError):
                jpeg.set_entropy(*args)
        assert jpeg.get_entropy() == dict(mode="parallel", subseq_bytes=64, max_rounds=9)
        with pytest.raises(ValueError):
            jpeg.get_entropy("fast")
    finally:
        jpeg.set_entropy(keep["mode"], keep["subseq_bytes"], keep["max_rounds"])
    im = jpeg_cases.image(NAMES[0])
    for args in ((8, 4), (20, 4), (8192, 4), (256, 0)):
        with pytest.raises(ValueError):
            im.parallel_plan(*args)


def test_the_fixtures_exercise_the_boundaries():
    """subsequence boundaries between FF and its stuffed 00, inside a restart marker, directly after and directly before one"""
    assert len(NAMES) == 74
    for size in (16, 24):
        many = stuffed = inside = after = before = 0
        for name in NAMES:
            p = jpeg_cases.image(name).entropy_bytes()
            many += -(-len(p) // size) >= 3
            for g in range(size, len(p), size):
                stuffed += p[g - 1] == 0xFF and p[g] == 0
                inside += p[g - 1] == 0xFF and 0xD0 <= p[g] <= 0xD7
                after += g >= 2 and p[g - 2] == 0xFF and 0xD0 <= p[g - 1] <= 0xD7
                before += g + 1 < len(p) and p[g] == 0xFF and 0xD0 <= p[g + 1] <= 0xD7
        print("subseq_bytes %d: %d files with >= 3 subsequences, boundaries: %d in FF 00, %d inside a marker, %d after, %d before"
              % (size, many, stuffed, inside, after, before))
        assert many >= 1 and stuffed >= 1 and inside >= 1 and after >= 1 and before >= 1, size


@pytest.mark.parametrize("size", SIZES)
def test_parallel_plan_agrees_with_coefficients(size):
    """with as many rounds as subsequences every fixture file converges and is clean, the write pass of the plan gives the
    coefficients of the sequential rule, and the live subsequences hold the file's blocks"""
    slow = 0
    for name in NAMES:
        im = jpeg_cases.image(name)
        nsub = subsequences(im, size)
        plan = im.parallel_plan(size, nsub, coefficients=True)
        want = im.coefficients()
        assert plan["fallback"] == 0 and plan["subsequences"] == nsub and 1 <= plan["rounds"] <= nsub, (name, plan)
        assert 1 <= plan["live"] <= nsub and len(plan["blocks"]) == plan["live"], (name, plan)
        assert sum(plan["blocks"]) == want.shape[0], name
        assert plan["decodes"] >= nsub
        assert plan["coefficients"].dtype == np.int16 and np.array_equal(plan["coefficients"], want), name
        slow = max(slow, plan["rounds"])
    assert slow > 2


def test_two_rounds_are_too_few_for_some_files():
    hit = 0
    for name in NAMES:
        im = jpeg_cases.image(name)
        plan = im.parallel_plan(16, 2)
        assert plan["rounds"] <= 2 and plan["fallback"] in (0, 1 << 16), (name, plan)
        full = im.parallel_plan(16, subsequences(im, 16))
        assert (plan["fallback"] != 0) == (full["rounds"] > 2), name
        if plan["fallback"]:
            assert plan["rounds"] == 2 and plan["live"] == 0 and "coefficients" not in im.parallel_plan(16, 2, coefficients=True)
        hit += plan["fallback"] == 1 << 16
    assert hit >= 1


def test_damaged_streams_are_not_clean():
    im = jpeg_cases.image("21x35_444_rst2")
    ent = im.entropy_bytes()
    first = ent.index(b"\xff\xd0")
    swapped = im.with_entropy(ent[:first] + b"\xff\xd1" + ent[first + 2:])
    for size in (16, 256):
        n = subsequences(im, size)
        assert im.parallel_plan(size, n)["fallback"] == 0
        for alt in (swapped, im.with_entropy(ent[:len(ent) // 2]), im.with_entropy(b""), im.with_entropy(ent[:2]),
                    im.with_entropy(ent[:first] + ent[first + 2:])):
            assert jpeg_cases.status_of(alt)[0] != 0
            assert alt.parallel_plan(size, n)["fallback"] == 1 << 17, (size, alt.name)


def test_parallel_scheme_under_the_sanitizers(tmp_path):
    """csrc/jpeg_sync.h compiled for the CPU with AddressSanitizer and UBSan, lanes simulated in order: the three FUZZ
    streams intact, truncated at every 7th byte and with 200 mutations each, at 16 and 256 bytes per subsequence, end
    clean; status and coefficient checksum of EVERY run are those of ``status_of`` (and of jpeg_decode_scan: the program
    compares); with as many rounds as subsequences an image is clean exactly when its stream decodes; rounds and fallback
    bits are what ``parallel_plan`` says on the intact streams and a sample of the damaged ones."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_parallel_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "instaorder_amd", "csrc"),
                            os.path.join(ROOT, "tests", "jpeg_parallel_host.cpp"), "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("the compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    ims = [jpeg_cases.image(n) for n in jpeg_cases.FUZZ]
    files = []
    for k, im in enumerate(ims):
        files.append(str(tmp_path / ("stream%d.bin" % k)))
        with open(files[-1], "wb") as f:
            f.write(jpeg_cases.stream_file(im))
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    rows = [ln.split() for ln in run.stdout.splitlines()]
    assert len(rows) == 2 * sum(2 + -(-im.nbytes_entropy // 7) + 200 for im in ims)
    clean = sum(r[6] == "0" for r in rows)
    assert 0 < clean < len(rows) and any(r[6] == "1" for r in rows) and any(r[6] == "2" for r in rows)
    checked = 0
    reference = {}                                               # (stream, kind, index) -> (image, status_of): the same at both sizes
    for s, size, kind, idx, max_rounds, rounds, fallback, status, checksum in rows:
        s, size, idx, max_rounds, rounds, fallback, status = (int(v) for v in (s, size, idx, max_rounds, rounds, fallback, status))
        ent = ims[s].entropy_bytes()
        if (s, kind, idx) not in reference:
            alt = ims[s] if kind == "I" else ims[s].with_entropy(ent[:idx] if kind == "T" else jpeg_cases.mutated(ent, idx))
            reference[(s, kind, idx)] = (alt, jpeg_cases.status_of(alt))
        alt, (want, csum) = reference[(s, kind, idx)]
        # EVERY run: the status and, where the stream decodes, the coefficients of the Python statement of the decoder
        assert status == want, (jpeg_cases.FUZZ[s], size, kind, idx, status, want)
        if want == 0:
            assert int(checksum) == csum, (jpeg_cases.FUZZ[s], size, kind, idx)
        # with as many rounds as subsequences every run converges, and an image is clean exactly when its stream decodes
        if max_rounds == max(1, -(-len(alt.entropy_bytes()) // size)):
            assert fallback in (0, 2) and (fallback == 0) == (status == 0), (jpeg_cases.FUZZ[s], size, kind, idx, fallback, status)
        else:
            assert kind == "I" and max_rounds == 2 and fallback in (0, 1)
        if not (kind == "I" or (kind == "T" and idx % 49 == 0) or (kind == "M" and idx < 40)):
            continue
        plan = alt.parallel_plan(size, max_rounds)
        assert (rounds, fallback << 16) == (plan["rounds"], plan["fallback"]), (jpeg_cases.FUZZ[s], size, kind, idx, plan)
        checked += 1
    assert checked >= 12 + 2 * 3 * 40
