"""Guards of tests/test_gpu_conv_edges.py that need no GPU.  The GPU cases were chosen for the arm of a launcher or kernel
that only their geometry selects; here the host-side predicates that pick those arms are restated (conv_edge_inputs.py,
each citing the function it restates) and every case is held to what its id names, so that a retuned threshold fails
here instead of letting the GPU case test something else.  Also: the by-hand exact-zero position sets against fp64
autograd, and the lattice decomposition of io_geom_dgrad (csrc/capi.hip) emulated in torch against autograd over the
whole case table."""
import pytest
import torch
import torch.nn.functional as F

import conv_edge_inputs as cei
from conv_edge_inputs import CASES, IDS

BY_ID = {v: k for k, v in IDS.items()}


def _fwd(i):
    return cei.geom_fwd(BY_ID[i])


def _dgrad(i):
    return cei.dgrad_classes(BY_ID[i])


def test_table_is_the_issue_table():
    assert len(CASES) == len(set(CASES)) == 29 and len(set(IDS.values())) == 29
    assert sum(1 for c in CASES if cei.GROUP[c] == "A") == 17
    assert sum(1 for c in CASES if cei.GROUP[c] == "B") == 6 and sum(1 for c in CASES if cei.GROUP[c] == "W") == 6
    for c in CASES:           # what every entry point requires of the channel counts (capi.hip, io_launch_conv_nt: 64 | C in bf16)
        assert c[3] % 64 == 0 and c[4] % 64 == 0 and min(cei.out_hw(c)) >= 1


# ---- io_geom_dgrad (capi.hip): classes, taps, extents ----------------------------------------------------------------------
def test_odd_map_classes_have_unequal_extent():
    c = BY_ID["odd-map-s2-3x3-unequal-classes"]
    assert cei.out_hw(c) == (8, 5)
    ext = {(ph, pw): (g["Ho"], g["Wo"], g["Th"], g["Tw"]) for ph, pw, g in cei.dgrad_classes(c)}
    assert ext == {(0, 0): (8, 5, 1, 1), (0, 1): (8, 4, 1, 2), (1, 0): (7, 5, 2, 1), (1, 1): (7, 4, 2, 2)}


def test_strided_1x1_has_three_classes_without_tap():
    cls = _dgrad("s2-1x1-odd-map-three-classes-without-tap")
    assert [(ph, pw) for ph, pw, g in cls if g["Th"] * g["Tw"] == 0] == [(0, 1), (1, 0), (1, 1)]
    g00 = cls[0][2]
    assert (g00["Th"], g00["Tw"], g00["Ho"], g00["Wo"]) == (1, 1, 4, 5) and cei.nt_nopad(g00)


def test_group_b_classes():
    s3 = _dgrad("abi-3x3-s3")                 # stride 3 on a 3x3: nine classes with one tap each
    assert len(s3) == 9 and all(g["Th"] == 1 and g["Tw"] == 1 for _, _, g in s3)
    s7 = {(ph, pw): (g["Th"], g["Tw"]) for ph, pw, g in _dgrad("abi-7x7-s2")}
    assert s7 == {(0, 0): (3, 3), (0, 1): (3, 4), (1, 0): (4, 3), (1, 1): (4, 4)}
    assert all(g["Th"] == 1 and g["Tw"] == 1 for _, _, g in _dgrad("abi-2x2-s2"))


# ---- io_launch_conv_nt (conv_igemm.hip): tile width, LIN, nopad, tails, IoFastDiv ---------------------------------------------
def test_tile_width_and_tails():
    f, r = _fwd("fwd-128-wide-67-row-tail-wgrad-short-split"), _dgrad("dgrad-128-wide-67-row-tail-wgrad-short-split")[0][2]
    for g in (f, r):
        assert cei.rows(g) == 2115 and cei.cdiv(2115, 128) * (g["Co"] // 128) == 272 > cei.NT_SMALL_TILES
        assert cei.nt_tile_width(g) == 128 and cei.nt_last_tile_rows(g) == 67
        assert not cei.nt_lin(g) and cei.nt_nopad(g)          # 128 !| M: the general 1x1 addressing
    assert cei.nt_tile_width(_dgrad("fwd-128-wide-67-row-tail-wgrad-short-split")[0][2]) == 64
    assert cei.nt_tile_width(_fwd("dgrad-128-wide-67-row-tail-wgrad-short-split")) == 64
    g = _fwd("128-wide-s2-3x3-odd-92x91-wgrad-27-splits")
    assert (g["Ho"], g["Wo"]) == (92, 91) and cei.nt_tile_width(g) == 128 and cei.nt_last_tile_rows(g) == 8372 - 65 * 128
    g = _fwd("3x3-maps-tile-spans-15-samples-m450")
    assert cei.rows(g) == 450 and cei.nt_last_tile_rows(g) == 66 and cei.nt_tile_width(g) == 64
    assert 127 // 9 + 1 == 15                                 # samples under the 128 rows of the first tile
    g = _fwd("1x1-maps-fastdiv-d1-two-row-tails")
    assert cei.rows(g) == 130 and cei.nt_last_tile_rows(g) == 2 and cei.fastdiv_d1(g) == (True, True)
    assert cei.fastdiv_d1(_dgrad("1x1-maps-fastdiv-d1-two-row-tails")[0][2]) == (True, True)
    g = _fwd("2x2-to-1x1-s2-3x3")
    assert (g["Ho"], g["Wo"]) == (1, 1) and cei.fastdiv_d1(g) == (True, True)
    assert [cei.fastdiv_d1(gg) for _, _, gg in _dgrad("2x2-to-1x1-s2-3x3")] == [(True, True)] * 4
    g = _fwd("one-column-map-wo1")
    assert (g["Ho"], g["Wo"]) == (9, 1) and cei.fastdiv_d1(g) == (False, True)


def test_padding_cases():
    g = _fwd("1x1-pad1-zero-border-not-nopad")
    assert (g["Ho"], g["Wo"]) == (7, 8) and not cei.nt_nopad(g) and not cei.nt_lin(g)
    assert (_fwd("3x3-pad2-output-larger")["Ho"], _fwd("3x3-pad2-output-larger")["Wo"]) == (7, 8)
    g = _fwd("s1-3x3-pad0-output-smaller")
    assert (g["Ho"], g["Wo"]) == (4, 9) and cei.wino_fwd_form(g)[0] == "direct" and not cei.wgrad_wino_shape_ok(g)


def test_winograd_forward_forms():
    want = {"wino-f23-2-wide": ("f23", None), "wino-f43-halo-at-96-4x4": ("f43-halo", 96),
            "wino-f43-halo-at-96-4x8": ("f43-halo", 96), "wino-f43-no-halo-128": ("f43", 128)}
    for i, form in want.items():
        assert cei.wino_fwd_form(_fwd(i)) == form, i
    assert [IDS[c] for c in cei.WINO_FWD] == list(want)
    for c in cei.WINO_FWD:                                    # their data gradient is the same form (3x3, stride 1, pad 1)
        (_, _, g), = cei.dgrad_classes(c)
        assert cei.wino_fwd_form(g) == cei.wino_fwd_form(cei.geom_fwd(c))


# ---- plan_wgrad / plan_wgrad_wino / io_launch_conv_wgrad (conv_igemm.hip) --------------------------------------------------------
def test_filter_gradient_plans():
    for i in ("fwd-128-wide-67-row-tail-wgrad-short-split", "dgrad-128-wide-67-row-tail-wgrad-short-split"):
        p = cei.plan_wgrad(_fwd(i))
        assert (p["splits"], p["kps"], p["last_split"], p["last_rows"]) == (8, 9, 4, 3), i
    p = cei.plan_wgrad(_fwd("128-wide-s2-3x3-odd-92x91-wgrad-27-splits"))
    assert (p["splits"], p["kps"], p["last_split"]) == (27, 10, 2)
    p = cei.plan_wgrad(_fwd("1x1-maps-fastdiv-d1-two-row-tails"))
    assert (p["nkt"], p["splits"], p["last_rows"]) == (5, 1, 2)
    for i, wo, form, splits in (("wgrad-tr-128x128-wo11-not-w4", 11, "tr", 2), ("wgrad-tr-128x128-wo10-not-w4-three-splits", 10, "tr", 3),
                                ("wgrad-tr-128x128-w4-s2-odd-ho17", 16, "tr-w4", 3)):
        g = _fwd(i)
        p = cei.plan_wgrad(g)
        assert g["Wo"] == wo and (p["bmo"], p["bnc"]) == (128, 128) and cei.wgrad_form(g, 0) == form, i
        assert p["splits"] == splits and cei.rows(g) % 32 != 0 and p["last_rows"] < 32, i
        assert cei.wgrad_form(g, 1) in ("rows", "w8")         # bf16: 64 !| Ho * Wo keeps them off the LDS-DMA kernel
    assert _fwd("wgrad-tr-128x128-w4-s2-odd-ho17")["Ho"] == 17
    g = _fwd("wo32-odd-ho7-wgrad-wino-row-or-w32")
    assert g["Ho"] == 7 and g["Wo"] == 32 and cei.wgrad_form(g, 0, True) == "wino-f43" and cei.wgrad_form(g, 0, False) == "rows-w32"
    assert cei.plan_wgrad_wino(g)["nkt"] == 7
    g = _fwd("wino-wgrad-f23-single-ktile")
    assert cei.wgrad_form(g, 0) == "wino-f23" and cei.plan_wgrad_wino(g) == dict(tiles=3, nkt=1, splits=1, kps=1)
    g = _fwd("wino-wgrad-f43-single-ktile")
    assert cei.wgrad_form(g, 0) == "wino-f43" and cei.plan_wgrad_wino(g) == dict(tiles=3, nkt=1, splits=1, kps=1)


def test_bf16_cases_stay_off_the_persistent_kernels():
    """no case of the table has conv_p256's / conv_halo3's shape in any pass: the GPU test asserts route 0 for all of them
    (the residual test reaches conv_p256 on purpose)"""
    for c in CASES:
        assert cei.bf16_nt_route(cei.geom_fwd(c)) == 0, IDS[c]
        assert all(cei.bf16_nt_route(g) == 0 for _, _, g in cei.dgrad_classes(c)), IDS[c]
        assert cei.bf16_wgrad_route(cei.geom_fwd(c)) == 0, IDS[c]
    taken = cei.geom_fwd((4, 8, 8, 256, 128, 1, 1, 1, 0))
    declined = cei.geom_fwd((4, 8, 8, 256, 64, 1, 1, 1, 0))
    assert cei.bf16_nt_route(taken) == 1 and cei.bf16_nt_route(declined) == 0
    assert [r[0][:5] + (r[2],) for r in cei.RESID if r[1] == 1] == [(4, 8, 8, 256, 64, 0), (4, 8, 8, 256, 128, 1)]


# ---- exact zeros ---------------------------------------------------------------------------------------------------------------
ZERO_DX = ["s2-3x3-pad0-last-row-col-unread", "s2-1x1-odd-map-three-classes-without-tap", "abi-2x2-s2"]


def test_zero_sets_are_where_the_ids_say():
    z = cei.dx_zero_positions(BY_ID["s2-3x3-pad0-last-row-col-unread"])
    want = torch.zeros(8, 10, dtype=torch.bool)
    want[7, :] = True
    want[:, 9] = True
    assert torch.equal(z, want)
    c = BY_ID["s2-1x1-odd-map-three-classes-without-tap"]
    z = cei.dx_zero_positions(c)
    assert int(z.sum()) == 7 * 9 - 4 * 5 and not bool(z[0::2, 0::2].any())
    assert torch.equal(z, cei.tapless_class_positions(c))
    yz = cei.y_zero_positions(BY_ID["1x1-pad1-zero-border-not-nopad"])
    want = torch.ones(7, 8, dtype=torch.bool)
    want[1:-1, 1:-1] = False
    assert torch.equal(yz, want)
    for c in CASES:
        if IDS[c] not in ZERO_DX:
            assert not bool(cei.tapless_class_positions(c).any()), IDS[c]
        # (pad 1 along a 1-wide filter axis: the first and last output rows / columns of the 1x3 / 3x1 cases too)
        assert bool(cei.y_zero_positions(c).any()) == (IDS[c] in ("1x1-pad1-zero-border-not-nopad", "abi-1x3", "abi-3x1")), IDS[c]


@pytest.mark.parametrize("case", CASES, ids=[IDS[c] for c in CASES])
def test_zero_sets_against_autograd_with_ones(case):
    """all-ones dy and filter: the gradient counts the windows that read a pixel, the output the taps inside the image --
    zero exactly on the by-hand sets"""
    N, H, W, Ci, Co, R, S, s, p = case
    x = torch.ones(1, 1, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.ones(1, 1, R, S, dtype=torch.float64)
    y = F.conv2d(x, w, stride=s, padding=p)
    gx, = torch.autograd.grad(y, x, torch.ones_like(y))
    assert torch.equal(gx[0, 0] == 0, cei.dx_zero_positions(case))
    assert torch.equal(y.detach()[0, 0] == 0, cei.y_zero_positions(case))


# ---- the lattice decomposition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[IDS[c] for c in CASES])
def test_lattice_emulation_matches_autograd(case):
    N, H, W, Ci, Co, R, S, s, p = case
    small = (2, H, W, 3, 2, R, S, s, p) if H * W <= 256 else (1, H, W, 1, 1, R, S, s, p)     # the geometry, few channels
    g = torch.Generator().manual_seed(H * W + R)
    x = torch.randn(small[0], small[3], H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(small[4], small[3], R, S, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, stride=s, padding=p)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    gx, = torch.autograd.grad(y, x, dy)
    got = cei.dgrad_by_lattice(small, dy, w)
    assert not bool(torch.isnan(got).any())                  # the classes cover every pixel
    assert float((got - gx).abs().max()) < 1e-12 * max(1.0, float(gx.abs().max()))
    assert bool((got[:, :, cei.dx_zero_positions(case)] == 0).all())
