"""COCO polygon masks on the host: ``poly.PolyMasks`` against an oracle written here from the published rule as sequential
code -- the concatenated walk of all edges, the crossing positions, a sort, run lengths with the zero-run merge, then a
fill per run.  That is a third formulation next to the package's per-edge vectorised ``to_dense()`` and the kernel's
parity planes (tests/test_gpu_poly.py imports the oracle and the polygon generator from here).  All comparisons are exact.
"""
import os

import numpy as np
import pytest

from helpers import ROOT
from instaorder_amd import _lib, poly, rle

IMAGES = [(1, 1), (1, 7), (7, 1), (5, 3), (61, 83)]


# ---- the oracle ------------------------------------------------------------------------------------------------------
def oracle_positions(flat, H, W):
    """the sorted crossing positions of one part, as the published C code finds them"""
    k = len(flat) // 2
    x = [int(5 * float(flat[2 * j]) + 0.5) for j in range(k)]            # int() truncates toward zero, as (int) does
    y = [int(5 * float(flat[2 * j + 1]) + 0.5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx == 0 and dy == 0:
            u.append(xs)
            v.append(ys)
            continue
        s = float(ye - ys) / dx if dx >= dy else float(xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    a = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j - 1])
        xd = (xd + .5) / 5 - .5
        if np.floor(xd) != xd or xd < 0 or xd > W - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / 5 - .5
        if yd < 0:
            yd = 0.0
        elif yd > H:
            yd = float(H)
        a.append(int(xd) * H + int(np.ceil(yd)))
    return sorted(a)


def oracle_part(flat, H, W):
    """bool [H, W] of one part: positions -> run lengths (zero-length runs merged) -> fill"""
    a = oracle_positions(flat, H, W) + [H * W]
    b, p = [], 0
    for q in a:
        b.append(q - p)
        p = q
    counts, j = [b[0]], 1
    while j < len(b):
        if b[j] > 0:
            counts.append(b[j])
            j += 1
        else:
            j += 1
            if j < len(b):
                counts[-1] += b[j]
                j += 1
    assert sum(counts) == H * W
    colmajor = np.zeros(H * W, bool)
    q, bit = 0, False
    for c in counts:
        colmajor[q:q + c] = bit
        q += c
        bit = not bit
    return colmajor.reshape(W, H).T.copy()


def oracle_mask(parts, H, W, value=1):
    m = np.zeros((H, W), bool)
    for flat in parts:
        m |= oracle_part(flat, H, W)
    return m.astype(np.uint8) * np.uint8(value)


# ---- polygons --------------------------------------------------------------------------------------------------------
def random_part(rs, H, W, style, k=None):
    """k (1..8) vertices: 'int' / 'half' / 'cent' = integer, half-integer and two-decimal coordinates reaching past the image
    on every side, 'neg' = mostly negative, 'left' / 'right' / 'above' / 'below' = wholly outside that side"""
    k = int(rs.randint(1, 9)) if k is None else k
    span = float(max(H, W))
    if style in ("int", "half", "cent"):
        xs = rs.uniform(-0.3 * span - 2, W + 0.3 * span + 2, k)
        ys = rs.uniform(-0.3 * span - 2, H + 0.3 * span + 2, k)
    elif style == "neg":
        xs, ys = rs.uniform(-W - 3, 0.4 * W, k), rs.uniform(-H - 3, 0.4 * H, k)
    else:
        xs, ys = rs.uniform(-2, W + 2, k), rs.uniform(-2, H + 2, k)
        if style == "left":
            xs = rs.uniform(-W - 6, -0.5, k)
        elif style == "right":
            xs = rs.uniform(W + 0.5, 2 * W + 6, k)
        elif style == "above":
            ys = rs.uniform(-H - 6, -0.5, k)
        else:
            ys = rs.uniform(H + 0.5, 2 * H + 6, k)
    digits = {"int": 0, "half": None, "cent": 2}.get(style, int(rs.randint(0, 3)))
    if digits is None:
        xs, ys = np.round(xs * 2) / 2, np.round(ys * 2) / 2
    else:
        xs, ys = np.round(xs, digits), np.round(ys, digits)
    return np.stack([xs, ys], axis=1).reshape(-1).tolist()


STYLES = ("int", "half", "cent", "neg", "left", "right", "above", "below")


def random_instances(seed, H, W, n):
    """n instances of 0..3 parts in every style"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        nparts = (1, 1, 2, 3, 0, 1)[i % 6]
        out.append([random_part(rs, H, W, STYLES[(i + p) % len(STYLES)], k=1 + (i // 8 + 3 * p) % 8) for p in range(nparts)])
    return out


VECTORS = [
    (4, 6, [1, 1, 4, 1, 4, 3, 1, 3], [5, 7, 9, 11, 13, 15], ["000000", "011100", "011100", "000000"]),
    (6, 7, [0.5, 0.5, 6.5, 1.0, 2.0, 5.5], [7, 10, 13, 17, 19, 22, 25, 27, 31, 32, 37, 37],
     ["0000000", "0111110", "0111100", "0111000", "0010000", "0000000"]),
    (6, 5, [-2, -1, 5, 2, 1, 8], [0, 6, 7, 12, 13, 18, 19, 22, 26, 27], ["10000", "11110", "11111", "11110", "11100", "11100"]),
    (4, 4, [2, 2], [], ["0000"] * 4),
    (5, 5, [1, 1, 4, 3], [6, 6, 12, 12, 18, 18], ["00000"] * 5),
]


def coco_string(counts):
    """the compressed string form of COCO run lengths (the published rleToString)"""
    out = []
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rows(mask):
    return ["".join("1" if v else "0" for v in r) for r in np.asarray(mask)]


# ---- tests -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(VECTORS)))
def test_fixed_vectors(k):
    """positions and masks of the five vectors of the rule: the oracle, the package's positions and ``to_dense()``"""
    H, W, flat, a, want = VECTORS[k]
    assert oracle_positions(flat, H, W) == a
    assert rows(oracle_part(flat, H, W)) == want
    pm = poly.PolyMasks([[flat]], H, W)
    assert pm.shape == (1, H, W) and pm.is_polygon(0)
    assert sorted(poly._part_positions(pm.parts(0)[0], H, W).tolist()) == a
    assert rows(pm.to_dense()[0]) == want


@pytest.mark.parametrize("size", IMAGES)
def test_to_dense_equals_oracle_on_a_sweep(size):
    """80 instances per image size (400 in all): 1..8 vertices, every coordinate style, polygons outside each side,
    multi-part instances (overlapping and disjoint as they fall) and instances with no parts"""
    H, W = size
    inst = random_instances(100 * H + W, H, W, 80)
    assert any(len(p) == 0 for p in inst) and any(len(p) == 3 for p in inst)
    values = [1 + (i * 37) % 255 for i in range(len(inst))]
    dense = poly.PolyMasks(inst, H, W, values=values).to_dense()
    assert dense.dtype == np.uint8 and dense.shape == (len(inst), H, W)
    filled = 0
    for i, parts in enumerate(inst):
        want = oracle_mask(parts, H, W, values[i])
        assert np.array_equal(dense[i], want), (size, i, parts)
        filled += int(want.any())
    print("instances with a pixel set:", filled)
    assert filled >= (4 if H * W == 1 else 10), "the sweep barely sets a pixel"


def test_overlapping_and_disjoint_parts_are_a_union():
    H, W = 20, 30
    a, b, c = [2, 2, 12, 2, 12, 12, 2, 12], [8, 6, 20, 6, 20, 16, 8, 16], [22, 1, 28, 1, 28, 5, 22, 5]
    m = poly.PolyMasks([[a, b], [a, c], [a], [b], [c]], H, W).to_dense().astype(bool)
    assert (m[2] & m[3]).any() and not (m[2] & m[4]).any()
    assert np.array_equal(m[0], m[2] | m[3]) and np.array_equal(m[1], m[2] | m[4])
    assert np.array_equal(m[0], oracle_mask([a, b], H, W).astype(bool))


def test_from_coco_takes_the_three_forms_of_one_image():
    """a polygon list, a run-length dict with a counts list and one with the compressed string, mixed in one image, as
    annotations and as bare segmentations; the run-length instances equal RLEMasks"""
    H, W = 5, 4
    crowd = {"size": [H, W], "counts": [3, 4, 6, 2, 5]}
    strobj = {"size": [H, W], "counts": coco_string([0, 2, 5, 1, 9, 3])}
    assert rle._counts_from_string(strobj["counts"]) == [0, 2, 5, 1, 9, 3]
    polygon = [[0.5, 0.5, 3.5, 0.5, 3.5, 4.5, 0.5, 4.5]]
    anns = [{"segmentation": polygon, "iscrowd": 0}, {"segmentation": crowd, "iscrowd": 1}, {"segmentation": strobj, "iscrowd": 1}]
    for src in (anns, [a["segmentation"] for a in anns]):
        pm = poly.PolyMasks.from_coco(src, H, W, values=[1, 9, 3])
        assert pm.shape == (3, H, W) and [pm.is_polygon(i) for i in range(3)] == [True, False, False]
        ref = rle.RLEMasks.from_coco([crowd, strobj], values=[9, 3]).to_dense()
        d = pm.to_dense()
        assert np.array_equal(d[1:], ref) and ref[0].max() == 9 and ref[1].max() == 3
        assert np.array_equal(d[0], oracle_mask(polygon, H, W))
        r, j = pm.rle_ref(1)
        assert isinstance(r, rle.RLEMasks) and int(r.values[j]) == 9 and pm.rle_ref(0) is None
    as_bytes = poly.PolyMasks.from_coco([dict(strobj, counts=strobj["counts"].encode("ascii"))], H, W, values=[3])
    assert np.array_equal(as_bytes.to_dense()[0], ref[1])
    with pytest.raises(ValueError, match="size"):
        poly.PolyMasks.from_coco([{"size": [H, W + 1], "counts": [H * (W + 1)]}], H, W)
    with pytest.raises(ValueError, match="flat list"):
        poly.PolyMasks.from_coco([[1.0, 2.0, 3.0, 4.0]], H, W)
    with pytest.raises(ValueError, match="counts"):
        poly.PolyMasks.from_coco([{"size": [H, W]}], H, W)
    with pytest.raises(ValueError):
        poly.PolyMasks.from_coco([7], H, W)


def test_indexing_and_with_values():
    H, W = 9, 11
    inst = random_instances(5, H, W, 5) + [{"size": [H, W], "counts": [10, 20, H * W - 30]}]
    pm = poly.PolyMasks(inst, H, W, values=[1, 2, 3, 4, 5, 6])
    d = pm.to_dense()
    assert len(pm) == 6 and list(pm.values) == [1, 2, 3, 4, 5, 6]
    assert pm[2].shape == (1, H, W) and np.array_equal(pm[2].to_dense()[0], d[2])
    assert np.array_equal(pm[-1].to_dense()[0], d[5]) and not pm[-1].is_polygon(0)
    assert np.array_equal(pm[1:4].to_dense(), d[1:4])
    assert np.array_equal(pm[[5, 0, 0]].to_dense(), d[[5, 0, 0]])
    keep = np.array([True, False, True, False, False, True])
    assert np.array_equal(pm[keep].to_dense(), d[keep])
    assert pm[[]].shape == (0, H, W) and pm[[]].to_dense().shape == (0, H, W)
    with pytest.raises(IndexError):
        pm[6]
    with pytest.raises(IndexError):
        pm[np.array([True, False])]
    with pytest.raises(IndexError):
        pm[1.5]
    w = pm.with_values([7, 7, 8, 8, 250, 255])
    assert np.array_equal(w.to_dense(), (d != 0) * np.array([7, 7, 8, 8, 250, 255], np.uint8)[:, None, None])
    assert np.array_equal(pm.to_dense(), d), "with_values changed the masks it was called on"
    assert np.array_equal(pm.with_values(9).to_dense(), (d != 0) * np.uint8(9))
    assert int(w.rle_ref(5)[0].values[0]) == 255 and int(pm.rle_ref(5)[0].values[0]) == 6
    assert w.parts(0)[0] is pm.parts(0)[0], "with_values copies the vertices"
    assert isinstance(pm, rle.EncodedMasks) and rle.is_encoded(pm) and rle.is_encoded(rle.RLEMasks([[4]], 2, 2))
    assert not rle.is_encoded(d)


def test_every_value_error():
    sq = [1, 1, 3, 1, 3, 3]
    for bad, what in (([[sq + [1]]], "even length"), ([[[]]], "even length"), ([[[1.0]]], "even length"),
                      ([[[1, 1, float("nan"), 2]]], "not finite"), ([[[1, 1, float("inf"), 2]]], "not finite"),
                      ([[[1, 1, 2.0 ** 24 / 5 + 1, 2]]], "beyond"), ([[[-2.0 ** 24, 1, 3, 2]]], "beyond"),
                      ([[1.5, 2.5, 3.5, 4.5]], "LIST of parts"), ([[[[1, 2], [3, 4]]]], "even length")):
        with pytest.raises(ValueError, match=what):
            poly.PolyMasks(bad, 8, 8)
    poly.PolyMasks([[[1, 1, 2.0 ** 24 / 5, 2]]], 8, 8)                      # the bound itself is taken
    for H, W in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15)):
        with pytest.raises(ValueError, match="size"):
            poly.PolyMasks([[sq]], H, W)
    for v in (256, -1, [1, 300], 1.0):
        with pytest.raises(ValueError, match="values"):
            poly.PolyMasks([[sq], [sq]], 8, 8, values=v)
        with pytest.raises(ValueError, match="values"):
            poly.PolyMasks([[sq], [sq]], 8, 8).with_values(v)
    with pytest.raises(ValueError, match="sum to"):                         # what RLEMasks refuses
        poly.PolyMasks([{"size": [8, 8], "counts": [3, 4]}], 8, 8)
    with pytest.raises(ValueError, match="negative"):
        poly.PolyMasks([[70, -6]], 8, 8)
    with pytest.raises(ValueError, match="run-length"):
        poly.PolyMasks([[64]], 8, 8).parts(0)
    assert poly.PolyMasks([[]], 8, 8).to_dense().sum() == 0                 # no parts: an empty mask


def test_symbols_structures_and_header():
    hdr = open(os.path.join(ROOT, "include", "instaorder_hip.h")).read()
    assert "int io_poly_fill_u8(" in hdr and "} io_poly_part;" in hdr and "} io_poly_mask;" in hdr
    assert "#define IO_POLY_SCAN_WORDS" in hdr
    assert len(_lib.SIGNATURES["io_poly_fill_u8"][1]) == 13
    assert len(_lib.SIGNATURES["io_poly_fill_workspace_bytes"][1]) == 4
    import ctypes as C
    assert C.sizeof(_lib.PolyPart) == 16 and C.sizeof(_lib.PolyMask) == 32
    lib = _lib.lib()
    assert poly.scan_words() == int(hdr.split("#define IO_POLY_SCAN_WORDS")[1].split()[0])
    assert int(hdr.split("#define IO_POLY_MAX_COORD (1 << ")[1].split(")")[0]) == 24 and poly.MAX_SCALED == 1 << 24
    # the planning call needs no GPU: a header of one offset per part, then one plane of ceil(H W / 32) words per part
    pm = poly.PolyMasks([[[1, 1, 5, 1, 5, 5], [0, 0, 1, 1]], [], [[2, 2]]], 7, 9)
    verts, parts, masks, n_parts = poly.descriptors([(pm, i) for i in range(3)], [0, 63, 126])
    assert n_parts == 3 and verts.shape == (6, 2) and verts.dtype == np.int32
    assert [(p.vert_off, p.n_verts, p.mask) for p in parts[:3]] == [(0, 3, 0), (3, 2, 0), (5, 1, 2)]
    assert [(m.first_part, m.n_parts, m.out_off) for m in masks] == [(0, 2, 0), (2, 0, 63), (2, 1, 126)]
    assert poly.workspace_bytes(parts, n_parts, masks) == 32 + 3 * 4 * 2
    parts[1].mask = 1
    assert lib.io_poly_fill_workspace_bytes(C.cast(parts, C.c_void_p), 3, C.cast(masks, C.c_void_p), 3) == 0
    assert "part 1" in _lib.last_error()
