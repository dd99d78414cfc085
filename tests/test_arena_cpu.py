"""The input pipeline's shared layout (instaorder_amd/arena.py) and the codec groups built on it, without a GPU: the
16-byte rule, the blobs of every group against the ``descriptors*`` functions they are built on -- with the aliasing the
renderer relies on when it sets the out-offsets late -- the empty groups, and source checks in the manner of
tests/test_ops_layer_cpu.py: one call site per decode entry point, one copy of the alignment expression."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpeg_cases
import jpeg_prog_cases
import png_cases
from helpers import ROOT
from instaorder_amd import arena, jpeg, png, poly, rle

SIZES = [0, 1, 15, 16, 17, 5, 0, 33, 16, 0]          # empty blobs first, between two non-empty ones and last


def test_layout_offsets_are_aligned_increasing_and_covered():
    lay = arena.Layout()
    assert lay.size == 0
    ats = [lay.add(n) for n in SIZES]
    assert ats[0] == 0 and all(a % 16 == 0 for a in ats)
    assert all(b > a for a, b in zip(ats, ats[1:]))                                # strictly: an empty blob has a place too
    assert all(a + n <= b for a, n, b in zip(ats, SIZES, ats[1:]))                 # no blob reaches into the next
    assert all(b - a == -(-max(n, 1) // 16) * 16 for a, n, b in zip(ats, SIZES, ats[1:]))     # the size rounded up, no more
    assert lay.size >= ats[-1] + SIZES[-1] and lay.size % 16 == 0
    for n, want in ((0, 16), (1, 16), (15, 16), (16, 16), (17, 32)):
        one = arena.Layout()
        assert one.add(n) == 0 and one.size == want == arena.room(n)


def test_pack_puts_each_blob_at_its_offset_and_zeroes_the_gaps():
    rng = np.random.RandomState(3)
    blobs = [rng.randint(1, 256, n).astype(np.uint8) for n in SIZES]              # no zero byte inside a blob
    host, ats = arena.pack(blobs)
    lay = arena.Layout()
    assert ats == [lay.add(n) for n in SIZES] and host.size == lay.size and host.dtype == np.uint8
    covered = np.zeros(host.size, bool)
    for a, b in zip(ats, blobs):
        assert np.array_equal(host[a:a + b.size], b)
        covered[a:a + b.size] = True
    assert not host[~covered].any() and host[covered].all()
    # into a buffer that is there already (the renderer's staging buffer, full of an earlier batch), at offsets of a
    # layout that holds other things in front
    lay = arena.Layout()
    lay.add(40)
    ats = [lay.add(b.size) for b in blobs]
    stage = np.full(lay.size + 64, 0xAB, np.uint8)
    same, same_ats = arena.pack(blobs, ats, stage)
    assert same is stage and same_ats is ats
    for a, b in zip(ats, blobs):
        assert np.array_equal(stage[a:a + b.size], b)
        assert not stage[a + b.size:a + arena.room(b.size)].any()
    assert (stage[:ats[0]] == 0xAB).all() and (stage[lay.size:] == 0xAB).all()     # nothing outside the blobs' room


def _poly_masks():
    H, W = 24, 40
    return poly.PolyMasks([[[2.5, 3.0, W - 3.0, 4.5, W / 2, H - 2.0]], {"size": [H, W], "counts": [50, 70, H * W - 120]},
                           [[-4, -3, W + 2, H / 2, 3, H + 5], [1, 1, 5, 1, 5, 5]], [0, 7, H * W - 7]], H, W,
                          values=[1, 2, 9, 3])


def _groups():
    """name -> (group, the arrays of the ``descriptors*`` function it is built on in blob order, workspace bytes or 0)"""
    base = [jpeg_cases.image(n) for n in ("33x47_420_q85", "40x24_422_q85", "21x35_444_q85")]
    prog = [jpeg_prog_cases.image(n) for n in ("33x47_420_q85", "33x47_420_lumafirst")]
    pngs = [png_cases.build(9, 13, "rgb", "mix", name="a.png")[0], png_cases.build(4, 7, "gray", "mix", name="b.png")[0]]
    pm = _poly_masks()
    rm = rle.RLEMasks([[0, 5, 19], [24], [7, 1, 16]], 4, 6, values=[1, 1, 5])
    rle_refs = [(rm, 2), pm.rle_ref(1), (rm, 0), pm.rle_ref(3)]
    poly_refs = [(pm, 2), (pm, 0)]
    zeros = lambda refs: [0] * len(refs)
    out = {}
    ends, rdesc = rle.descriptors(rle_refs, zeros(rle_refs))
    out["rle"] = (rle.group(rle_refs), [ends, rdesc], 0)
    verts, parts, masks, n_parts = poly.descriptors(poly_refs, zeros(poly_refs))
    out["poly"] = (poly.group(poly_refs), [verts, parts, masks], poly.workspace_bytes(parts, n_parts, masks))
    for mode in ("sequential", "parallel"):
        pool, tables, jdesc = jpeg.descriptors(base, zeros(base))
        out["jpeg " + mode] = (jpeg.group(base, mode), [pool, tables, jdesc], jpeg.workspace_bytes(jdesc, mode))
        gpool, gdesc = png.descriptors(pngs, zeros(pngs))
        out["png " + mode] = (png.group(pngs, mode), [gpool, gdesc], png.workspace_bytes(gdesc, mode))
    p = jpeg.descriptors_progressive(prog, zeros(prog))
    out["progressive"] = (jpeg.group_progressive(prog, 1), jpeg.progressive_blobs(p), jpeg.workspace_bytes_progressive(p))
    return out, dict(rle=0, poly=0, jpeg=len(base), png=len(pngs), progressive=len(prog))


def _raw(a):
    return a.view(np.uint8).reshape(-1) if isinstance(a, np.ndarray) else np.frombuffer(a, dtype=np.uint8)


@pytest.mark.parametrize("name", ["rle", "poly", "jpeg sequential", "jpeg parallel", "png sequential", "png parallel",
                                  "progressive"])
def test_group_blobs_are_the_descriptor_functions_arrays_and_alias_the_outs(name):
    groups, n_status = _groups()
    g, want, ws = groups[name]
    assert len(g.blobs) == len(want) == len(g.classes) and len(g) == len(g.outs) > 0
    for b, w in zip(g.blobs, want):
        assert b.dtype == np.uint8 and b.ndim == 1 and np.array_equal(b, _raw(w))
    assert set(g.classes) <= {"images", "masks", "descriptors"}
    assert ("masks" in g.classes) == (name in ("rle", "poly")) and ("images" in g.classes) == (name not in ("rle", "poly"))
    assert g.n_status == n_status[name.split()[0]] == len(g.images)
    if g.n_status:
        assert g.raise_for_status is (png if name.startswith("png") else jpeg).raise_for_status
        g.raise_for_status([0] * g.n_status, g.images)
        with pytest.raises(RuntimeError, match=g.images[-1].name):
            g.raise_for_status([0] * (g.n_status - 1) + [1], g.images)
    assert g.workspace_bytes() == ws and (ws > 0) == (name != "rle")
    # the out-offsets are set after the blobs exist: the descriptor blob shows them (what the renderer uploads)
    which = [b for b, c in zip(g.blobs, g.classes) if c == "descriptors" and b.size == C.sizeof(g.outs)]
    assert len(which) == 1
    before = which[0].copy()
    offs = [1000 * 16 + 4096 * k for k in range(len(g))]
    g.set_outs(offs)
    assert [g.outs[k].out_off for k in range(len(g))] == offs
    assert not np.array_equal(which[0], before) and np.array_equal(which[0], np.frombuffer(g.outs, dtype=np.uint8))
    g.outs[0].out_off = 48
    assert np.array_equal(which[0], np.frombuffer(g.outs, dtype=np.uint8)) and g.outs[0].out_off == 48
    g.set_outs([0] * len(g))
    assert np.array_equal(which[0], before)


def test_a_group_without_members_is_empty():
    for g in (rle.group([]), poly.group([]), jpeg.group([], "sequential"), jpeg.group([], "parallel"), jpeg.group([], None),
              jpeg.group_progressive([], None), jpeg.group_progressive([], 0), png.group([], "sequential"),
              png.group([], "parallel")):
        assert len(g) == 0 and g.blobs == [] and g.classes == () and g.n_status == 0 and g.workspace_bytes() == 0
        assert g.images == [] and len(g.outs) == 0


def _package_sources():
    d = os.path.join(ROOT, "instaorder_amd")
    out = {}
    for fn in sorted(os.listdir(d)):
        if fn.endswith(".py"):
            with open(os.path.join(d, fn)) as f:
                out[fn] = f.read()
    return out


@pytest.mark.parametrize("name", ["io_rle_decode_u8", "io_poly_fill_u8", "io_jpeg_decode_u8", "io_jpeg_decode_par_u8",
                                  "io_jpeg_decode_prog_u8", "io_png_decode", "io_png_decode_par", "io_pair_planes_u8_hw"])
def test_entry_point_has_one_call_site_in_the_package(name):
    sites = [(fn, m.start()) for fn, src in _package_sources().items()
             for m in re.finditer(r"\.%s\(" % re.escape(name), src)]
    assert len(sites) == 1, (name, sites)
    home = {"io_rle_decode_u8": "rle.py", "io_poly_fill_u8": "poly.py", "io_png_decode": "png.py", "io_png_decode_par": "png.py",
            "io_pair_planes_u8_hw": "datasets.py"}.get(name, "jpeg.py")
    assert sites[0][0] == home


def test_the_alignment_expression_lives_in_arena_only():
    src = _package_sources()
    counts = {fn: src[fn].count("+ 15) // 16 * 16") for fn in ("datasets.py", "rle.py", "poly.py", "jpeg.py", "png.py", "arena.py")}
    assert counts == {"datasets.py": 0, "rle.py": 0, "poly.py": 0, "jpeg.py": 0, "png.py": 0, "arena.py": 1}, counts
    for fn in ("datasets.py", "rle.py", "poly.py", "jpeg.py", "png.py"):
        assert not re.search(r"//\s*16\s*\*\s*16", src[fn]), fn                   # nor the rule in another spelling
